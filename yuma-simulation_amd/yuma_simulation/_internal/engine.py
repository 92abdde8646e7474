"""ctypes binding of libyuma_hip.so (include/yuma_hip.h) — the only compute path.

The product never falls back to CPU: if the HIP library or a GPU is missing,
every compute entry point raises ``EngineUnavailable``. Tensors are handed over
as raw device pointers; the engine is stream-ordered on torch's current stream
and allocates nothing (the workspace is a torch uint8 tensor).

Parameter marshalling mirrors how the reference's torch ops round Python
scalars (yumas.py:7-45 configs, used at :186-262 and copies):
  * a Python float meeting an fp32 tensor is rounded to fp32 first;
  * ``1 - x`` of two Python floats is computed in double, then rounded;
  * the bisection trip count is the reference's own loop evaluated in double.
"""

from __future__ import annotations

import ctypes
import math
import numbers
import operator
import os
import threading
from dataclasses import dataclass

import numpy as np
import torch

LIB_NAME = "libyuma_hip.so"
_PKG_ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
LIB_PATH = os.environ.get("YUMA_HIP_LIB", os.path.join(_PKG_ROOT, "lib", LIB_NAME))

VARIANT_RUST, VARIANT_YUMA1, VARIANT_YUMA2, VARIANT_YUMA3, VARIANT_YUMA4 = range(5)
PHASES = ("rowsum", "consensus", "quantise", "rank", "incentive", "bonds", "finalize")
FLAG_NO_HIST = 1  # yuma_params_t.flags: plain bisection instead of the histogram finish
FLAG_RESET_ALL_COLUMNS = 2  # the reset zeroes every column (reset_bonds_index None)
RESET_NONE, RESET_ALWAYS, RESET_IF_ZERO_CONSENSUS = range(3)
RUN_SHARED_INPUTS = 1  # yuma_run_ex flags
RUN_W_U16 = 2  # ... W holds uint16 elements (the on-chain weight format), read natively
RUN_HIST_BF16 = 4  # ... B_hist holds bfloat16 elements, written by the bond scan
LIQUID_OFF, LIQUID_QUANTILE, LIQUID_CONST_AB = range(3)
OVR_HIGH, OVR_LOW, OVR_FORCE_Q99 = 1, 2, 4
PAIRS_UPSCALE = 1  # yuma_weights_from_pairs flags
PAIRS_ST_DROPPED, PAIRS_ST_CONFLICT_ROWS, PAIRS_ST_BAD_ROWS, PAIRS_ST_WORDS = 0, 1, 2, 4  # ... its status words

EXPORTED_SYMBOLS = (
    "yuma_workspace_bytes",
    "yuma_run",
    "yuma_run_profiled",
    "yuma_run_ex",
    "yuma_run_opts",
    "yuma_hist_slots",
    "yuma_workspace_bytes_sched",
    "yuma_run_sched",
    "yuma_sched_native",
    "yuma_graph_create_sched",
    "yuma_run_watch",
    "yuma_watch_native",
    "yuma_graph_create_watch",
    "yuma_run_move",
    "yuma_move_native",
    "yuma_graph_create_move",
    "yuma_run_rows",
    "yuma_rows_native",
    "yuma_graph_create_rows",
    "yuma_workspace_bytes_rowstat",
    "yuma_run_rowstat",
    "yuma_rowstat_native",
    "yuma_graph_create_rowstat",
    "yuma_workspace_bytes_resets",
    "yuma_run_resets",
    "yuma_resets_native",
    "yuma_graph_create_resets",
    "yuma_workspace_bytes_events",
    "yuma_run_events",
    "yuma_events_native",
    "yuma_graph_create_events",
    "yuma_run_request",
    "yuma_graph_create_request",
    "yuma_workspace_bytes_request",
    "yuma_scan_plan",
    "yuma_epoch",
    "yuma_synth_weights",
    "yuma_weights_from_pairs",
    "yuma_shard_stage",
    "yuma_graph_create",
    "yuma_graph_create_ex",
    "yuma_graph_create_opts",
    "yuma_graph_launch",
    "yuma_graph_nodes",
    "yuma_graph_destroy",
    "yuma_last_error",
    "yuma_version",
    "yuma_build_id",
)


class EngineUnavailable(RuntimeError):
    """The HIP engine cannot run here (library not built or no GPU)."""


class EngineError(RuntimeError):
    """The engine rejected a call (bad sizes, workspace, launch failure)."""


MAX_VALIDATORS = 1 << 20  # include/yuma_hip.h YUMA_MAX_VALIDATORS
REG_VALIDATORS = 1024  # YUMA_REG_VALIDATORS: above it the engine streams each miner column
MAX_BISECT_ITERS = 30  # consensus_precision <= 2**30: the search grid k / 2**iters in int32


def check_limits(V: int, M: int) -> None:
    """The engine's size limits, checked before anything touches a GPU. The
    reference (yumas.py:195-209) has none; real subnets stay far inside them
    (DESIGN.md §3 'Limits')."""
    if V > MAX_VALIDATORS:
        raise EngineError(f"{V} validators exceed the engine's limit of {MAX_VALIDATORS} per subnet "
                          "(YUMA_MAX_VALIDATORS)")
    if M > (1 << 20) * 64:
        raise EngineError(f"{M} miners exceed the engine's limit of {(1 << 20) * 64} (2^20 tiles of 64)")


class YumaParamsC(ctypes.Structure):
    _fields_ = [
        ("variant", ctypes.c_int32),
        ("bisect_iters", ctypes.c_int32),
        ("liquid_mode", ctypes.c_int32),
        ("override_flags", ctypes.c_int32),
        ("reset_mode", ctypes.c_int32),
        ("reset_epoch", ctypes.c_int32),
        ("reset_index", ctypes.c_int32),
        ("flags", ctypes.c_int32),
        ("kappa", ctypes.c_float),
        ("bond_penalty", ctypes.c_float),
        ("one_minus_bond_penalty", ctypes.c_float),
        ("bond_alpha", ctypes.c_float),
        ("one_minus_bond_alpha", ctypes.c_float),
        ("alpha_low", ctypes.c_float),
        ("alpha_high", ctypes.c_float),
        ("capacity_alpha", ctypes.c_float),
        ("decay_keep", ctypes.c_float),
        ("maxint", ctypes.c_float),
        ("const_a", ctypes.c_float),
        ("const_b", ctypes.c_float),
        ("ln_num", ctypes.c_double),
        ("ln_low", ctypes.c_double),
        ("override_high", ctypes.c_double),
        ("override_low", ctypes.c_double),
        ("reserved1", ctypes.c_double * 2),
    ]


assert ctypes.sizeof(YumaParamsC) == 128, ctypes.sizeof(YumaParamsC)

OUTPUT_FIELDS = (
    "Dn", "D", "C", "I", "R", "P", "T", "Tv", "Sn", "bond_alpha", "alpha_ab",
    "Wn", "Wc", "Wb", "B_inst", "B_hist", "B_final",
)


class YumaOutputsC(ctypes.Structure):
    _fields_ = [(name, ctypes.c_void_p) for name in OUTPUT_FIELDS]


SHARD_IO_FIELDS = ("rowsum_part", "rowsum", "csum_part", "csum_part_d", "csum", "csum_d",
                   "levels", "rsum_part", "rsum", "levels_all", "dsum_part", "dsum", "tv_part", "tv")


class YumaResetEventC(ctypes.Structure):
    """yuma_reset_event_t (include/yuma_hip.h): 16 bytes."""
    _fields_ = [("epoch", ctypes.c_int32), ("scenario", ctypes.c_int32), ("column", ctypes.c_int32),
                ("mode", ctypes.c_int32)]


assert ctypes.sizeof(YumaResetEventC) == 16, ctypes.sizeof(YumaResetEventC)


class YumaRowEventC(ctypes.Structure):
    """yuma_row_event_t (include/yuma_hip.h): 16 bytes."""
    _fields_ = [("epoch", ctypes.c_int32), ("scenario", ctypes.c_int32), ("row", ctypes.c_int32),
                ("reserved", ctypes.c_int32)]


assert ctypes.sizeof(YumaRowEventC) == 16, ctypes.sizeof(YumaRowEventC)


class YumaRunOptionsC(ctypes.Structure):
    """yuma_run_options_t (include/yuma_hip.h): 32 bytes."""
    _fields_ = [("flags", ctypes.c_int32), ("hist_stride", ctypes.c_int32), ("hist_first", ctypes.c_int32),
                ("reserved", ctypes.c_int32 * 5)]


assert ctypes.sizeof(YumaRunOptionsC) == 32, ctypes.sizeof(YumaRunOptionsC)


REQ_WATCH, REQ_MOVE, REQ_ROWS, REQ_ROWSTAT, REQ_RESETS, REQ_ROW_EVENTS = 1, 2, 4, 8, 16, 32  # yuma_request_sections


class YumaRequestC(ctypes.Structure):
    """yuma_request_t (include/yuma_hip.h): 256 bytes. A section is present by its REQ_* bit in `sections`."""
    _fields_ = ([("struct_size", ctypes.c_uint32), ("sections", ctypes.c_uint32)]
                + [(n, ctypes.c_int32) for n in ("variant", "N", "E", "K", "V", "M")]
                + [(n, ctypes.c_void_p) for n in ("params_dev", "W", "S", "sched_dev", "B_init", "Wprev_init", "out",
                                                  "workspace")]
                + [("workspace_bytes", ctypes.c_size_t)]
                + [(n, ctypes.c_void_p) for n in ("opts", "watch_dev", "B_watch", "B_move", "rows_dev", "B_rows",
                                                  "B_rowstat", "events_dev", "row_events_dev")]
                + [(n, ctypes.c_int32) for n in ("chunk_epochs", "n_watch", "n_rows", "n_events", "n_row_events")]
                + [("reserved", ctypes.c_int32 * 15)])


assert ctypes.sizeof(YumaRequestC) == 256, ctypes.sizeof(YumaRequestC)


class YumaShardIOC(ctypes.Structure):
    """yuma_shard_io_t (include/yuma_hip.h): two ints, then device pointers."""
    _fields_ = [("M_total", ctypes.c_int), ("col0", ctypes.c_int)] + [
        (name, ctypes.c_void_p) for name in SHARD_IO_FIELDS]


_lock = threading.Lock()
_lib = None


def load_library(path: str | None = None):
    """Load (once) and type the C-ABI library. Raises EngineUnavailable."""
    global _lib
    with _lock:
        if _lib is not None:
            return _lib
        p = path or os.environ.get("YUMA_LIB") or LIB_PATH  # YUMA_LIB: A/B of two builds (tools/ab_lib.sh)
        if not os.path.exists(p):
            raise EngineUnavailable(
                f"{LIB_NAME} not found at {p}; build it with `python -c 'import __graft_entry__ as g; g.build()'`"
            )
        try:
            lib = ctypes.CDLL(p)
        except OSError as e:  # pragma: no cover - depends on the ROCm runtime
            raise EngineUnavailable(f"cannot load {p}: {e}") from e
        vp, i32, sz = ctypes.c_void_p, ctypes.c_int, ctypes.c_size_t
        lib.yuma_workspace_bytes.argtypes = [i32, i32, i32, i32, i32, i32]
        lib.yuma_workspace_bytes.restype = sz
        lib.yuma_run.argtypes = [i32, vp, i32, i32, i32, i32, vp, vp, vp, vp, vp, vp, sz, i32, vp]
        lib.yuma_run.restype = i32
        lib.yuma_run_profiled.argtypes = lib.yuma_run.argtypes + [ctypes.POINTER(ctypes.c_float)]
        lib.yuma_run_profiled.restype = i32
        lib.yuma_run_ex.argtypes = lib.yuma_run.argtypes[:-1] + [i32, vp, ctypes.POINTER(ctypes.c_float)]
        lib.yuma_run_ex.restype = i32
        lib.yuma_run_opts.argtypes = lib.yuma_run.argtypes[:-1] + [vp, vp, ctypes.POINTER(ctypes.c_float)]
        lib.yuma_run_opts.restype = i32
        lib.yuma_hist_slots.argtypes = [i32, i32, i32]
        lib.yuma_hist_slots.restype = i32
        # (not in EXPORTED_SYMBOLS: that tuple mirrors the header scan of
        # test_host.py, whose pattern takes lower-case letters only)
        lib.yuma_u16_native.argtypes = [i32, i32, i32, i32, i32, vp, i32]
        lib.yuma_u16_native.restype = i32
        # (outside EXPORTED_SYMBOLS for the same reason: the digits in its name)
        if hasattr(lib, "yuma_hist_bf16_native"):  # (A/B libraries of older sources lack it)
            lib.yuma_hist_bf16_native.argtypes = [i32, i32, i32, i32, i32, vp, i32]
            lib.yuma_hist_bf16_native.restype = i32
        lib.yuma_epoch.argtypes = [i32, vp, i32, i32, i32, vp, vp, vp, vp, vp, vp, sz, vp]
        lib.yuma_epoch.restype = i32
        lib.yuma_shard_stage.argtypes = [i32, i32, vp, i32, i32, i32, i32, vp, vp, vp, vp, vp, vp,
                                         vp, sz, vp]
        lib.yuma_shard_stage.restype = i32
        lib.yuma_synth_weights.argtypes = [ctypes.c_uint64, i32, i32, i32, i32, i32, vp, vp]
        lib.yuma_synth_weights.restype = i32
        if hasattr(lib, "yuma_weights_from_pairs"):  # (A/B libraries of older sources lack it: the call refuses those)
            lib.yuma_weights_from_pairs.argtypes = [ctypes.c_longlong, i32, ctypes.c_longlong, vp, vp, vp, i32, vp,
                                                    vp, vp]
            lib.yuma_weights_from_pairs.restype = i32
        lib.yuma_graph_create.argtypes = [ctypes.POINTER(vp), i32, vp, i32, i32, i32, i32, vp, vp,
                                          vp, vp, vp, vp, sz, i32]
        lib.yuma_graph_create.restype = i32
        lib.yuma_graph_create_ex.argtypes = lib.yuma_graph_create.argtypes + [i32]
        lib.yuma_graph_create_ex.restype = i32
        lib.yuma_graph_create_opts.argtypes = lib.yuma_graph_create.argtypes + [vp]
        lib.yuma_graph_create_opts.restype = i32
        # The positional rungs: (name, base, position in the run's list, inserted types). Each rung's arguments are
        # its base's with a few spliced in; its graph twin's are the same one place on (the handle comes first).
        # With each, its yuma_<name>_native predicate and, where it has one, its yuma_workspace_bytes_<name>.
        fp = ctypes.POINTER(ctypes.c_float)
        if hasattr(lib, "yuma_run_sched"):  # input schedules: E and K in place of E, the schedule after S
            lib.yuma_run_sched.argtypes = [i32, vp, i32, i32, i32, i32, i32, vp, vp, vp, vp, vp, vp, vp, sz, i32, vp, vp, fp]
            lib.yuma_graph_create_sched.argtypes = [ctypes.POINTER(vp)] + lib.yuma_run_sched.argtypes[:-2]
        rungs = (
            ("watch", "sched", 13, [vp, i32, vp]),   # the list, its length and B_watch after `out`
            ("move", "watch", 16, [vp]),             # B_move after B_watch
            ("rows", "move", 17, [vp, i32, vp]),     # the row list, its length and B_rows after B_move
            ("rowstat", "rows", 20, [vp]),           # B_rowstat after B_rows
            ("resets", "opts", 11, [vp, i32]),       # the event list and its length after `out`
            ("events", "resets", 13, [vp, i32]),     # the row event list and its length after n_events
        )
        for name, base, at, ins in rungs:
            if not hasattr(lib, "yuma_run_" + name):  # (A/B libraries of older sources lack the later rungs)
                continue
            for prefix, k in (("yuma_run_", at), ("yuma_graph_create_", at + 1)):
                a = getattr(lib, prefix + base).argtypes
                getattr(lib, prefix + name).argtypes = a[:k] + ins + a[k:]
        by_out, by_count = [i32, i32, i32, i32, i32, vp, i32], [i32] * 7  # (..., out, flags) / (..., n, flags)
        native = {"sched": [i32] * 6 + [vp, i32], "watch": by_count, "move": by_out, "rows": by_count,
                  "rowstat": by_out, "resets": by_out, "events": by_out}
        for name, types in native.items():
            if not hasattr(lib, "yuma_run_" + name):
                continue
            getattr(lib, "yuma_run_" + name).restype = i32
            getattr(lib, "yuma_graph_create_" + name).restype = i32
            getattr(lib, f"yuma_{name}_native").argtypes = types
            getattr(lib, f"yuma_{name}_native").restype = i32
            if name in ("sched", "rowstat", "resets", "events"):
                fn = getattr(lib, "yuma_workspace_bytes_" + name)
                fn.argtypes, fn.restype = [i32] * (7 if name == "sched" else 6), sz
        if hasattr(lib, "yuma_run_request"):  # (A/B libraries of older sources lack them: _launch refuses those)
            lib.yuma_run_request.argtypes = [vp, vp, fp]
            lib.yuma_run_request.restype = i32
            lib.yuma_graph_create_request.argtypes = [ctypes.POINTER(vp), vp]
            lib.yuma_graph_create_request.restype = i32
            lib.yuma_workspace_bytes_request.argtypes = [vp]
            lib.yuma_workspace_bytes_request.restype = sz
        if hasattr(lib, "yuma_scan_plan"):  # (A/B libraries of older sources lack it)
            lib.yuma_scan_plan.argtypes = [i32, i32, i32, i32, i32, vp, vp, i32, i32, i32, vp]
            lib.yuma_scan_plan.restype = i32
        lib.yuma_graph_launch.argtypes = [vp, vp]
        lib.yuma_graph_launch.restype = i32
        lib.yuma_graph_nodes.argtypes = [vp]
        lib.yuma_graph_nodes.restype = i32
        lib.yuma_graph_destroy.argtypes = [vp]
        lib.yuma_graph_destroy.restype = i32
        lib.yuma_last_error.argtypes = []
        lib.yuma_last_error.restype = ctypes.c_char_p
        lib.yuma_version.argtypes = []
        lib.yuma_version.restype = ctypes.c_char_p
        if hasattr(lib, "yuma_build_id"):  # (A/B libraries of older sources lack it)
            lib.yuma_build_id.argtypes = []
            lib.yuma_build_id.restype = ctypes.c_char_p
        _lib = lib
        return lib


def device() -> torch.device:
    """The GPU the engine runs on; raises EngineUnavailable without one."""
    if not torch.cuda.is_available():
        raise EngineUnavailable("the Yuma HIP engine needs a ROCm GPU (torch.cuda.is_available() is False)")
    load_library()
    return torch.device("cuda", torch.cuda.current_device())


def _check(rc: int, what: str) -> None:
    if rc != 0:
        msg = load_library().yuma_last_error().decode(errors="replace")
        raise EngineError(f"{what} failed ({rc}): {msg}")


def _ptr(t: torch.Tensor | None) -> int | None:
    return None if t is None else t.data_ptr()


# ---------------------------------------------------------------------------
# parameter marshalling
# ---------------------------------------------------------------------------
def bisect_iterations(consensus_precision) -> int:
    """Trip count of `while (c_high - c_low) > 1 / precision` (yumas.py:201):
    the interval halves exactly every iteration, independent of the data."""
    threshold = 1 / consensus_precision
    hi, lo, n = 1.0, 0.0, 0
    while (hi - lo) > threshold:
        hi = (hi + lo) / 2.0
        n += 1
        if n > 4096:  # pragma: no cover - nonsensical precision
            raise ValueError("consensus_precision too large")
    return n


def f32(x) -> float:
    return float(np.float32(x))


def make_params(variant: int, config, *, maxint: int = 2**64 - 1, reset_mode: int = RESET_NONE,
                reset_epoch: int | None = None, reset_index: int | None = None,
                n_miners: int | None = None, n_epochs: int | None = None,
                resumed: bool = False) -> YumaParamsC:
    """Flatten a YumaConfig (yumas.py:29-45) into the engine's POD record.
    resumed: the run starts from a caller's B_init, so a bond state exists at
    epoch 0 and a reset at epoch 0 is reached (_pack_reset)."""
    p = YumaParamsC()
    p.variant = variant
    p.bisect_iters = bisect_iterations(config.consensus_precision)
    if p.bisect_iters > MAX_BISECT_ITERS:
        raise EngineError(f"consensus_precision {config.consensus_precision} needs {p.bisect_iters} bisection "
                          f"steps; the engine supports at most {MAX_BISECT_ITERS} (consensus_precision <= 2**30)")
    p.kappa = f32(config.kappa)
    p.bond_penalty = f32(config.bond_penalty)
    p.one_minus_bond_penalty = f32(1 - config.bond_penalty)
    p.bond_alpha = f32(config.bond_alpha)
    p.one_minus_bond_alpha = f32(1 - config.bond_alpha)
    p.alpha_low = f32(config.alpha_low)
    p.alpha_high = f32(config.alpha_high)
    p.capacity_alpha = f32(config.capacity_alpha)
    p.decay_keep = f32(1 - config.decay_rate)
    p.maxint = f32(float(maxint))
    p.const_a = p.const_b = float("nan")
    p.override_high = p.override_low = float("nan")
    p.liquid_mode = LIQUID_OFF
    uses_liquid = variant in (VARIANT_RUST, VARIANT_YUMA1, VARIANT_YUMA2, VARIANT_YUMA4)
    if config.liquid_alpha and uses_liquid:
        # the reference evaluates these when it reaches them (yumas.py:248-251);
        # math.log raises ValueError for alpha outside (0, 1) exactly as there
        ln_high = math.log(1 / config.alpha_high - 1)
        ln_low = math.log(1 / config.alpha_low - 1)
        p.ln_num = ln_high - ln_low
        p.ln_low = ln_low
        hi_o, lo_o = config.override_consensus_high, config.override_consensus_low
        flags = 0
        if hi_o is not None:
            flags |= OVR_HIGH
            p.override_high = float(hi_o)
        if lo_o is not None:
            flags |= OVR_LOW
            p.override_low = float(lo_o)
        p.liquid_mode = LIQUID_QUANTILE
        if hi_o is not None and lo_o is not None:
            if hi_o == lo_o:  # python comparison, then consensus_high = quantile(.99)
                flags |= OVR_FORCE_Q99
            else:  # pure-python a, b (doubles), rounded when they meet C
                a = (ln_high - ln_low) / (lo_o - hi_o)
                b = ln_low + a * lo_o
                p.const_a, p.const_b = f32(a), f32(b)
                p.liquid_mode = LIQUID_CONST_AB
        p.override_flags = flags
    _pack_reset(p, reset_mode, reset_epoch, reset_index, n_miners, n_epochs, resumed)
    return p


_PARAMS_CACHE: dict = {}
_CONFIG_FIELDS = ("consensus_precision", "kappa", "bond_penalty", "bond_alpha", "alpha_low", "alpha_high",
                  "capacity_alpha", "decay_rate", "liquid_alpha", "override_consensus_high",
                  "override_consensus_low")


def config_key(config) -> tuple:
    """The values make_params reads from a config (repr: -0.0 and 0.0 differ)."""
    return tuple(repr(getattr(config, f)) for f in _CONFIG_FIELDS)


def make_params_cached(variant: int, config, *, reset_mode: int = RESET_NONE, reset_epoch=None,
                       reset_index=None, n_miners: int | None = None, n_epochs: int | None = None,
                       ckey: tuple | None = None, resumed: bool = False) -> YumaParamsC:
    """make_params memoised on every value it reads (the sheet builds 504
    records from 36 distinct configurations). Plain int / None reset fields
    only; anything else (a tensor-valued reset epoch) is built fresh. The
    record is shared: callers copy it into the device tensor, never mutate it.
    ckey: config_key(config), when the caller already has it."""
    if not all(x is None or type(x) is int for x in (reset_epoch, reset_index)):
        return make_params(variant, config, reset_mode=reset_mode, reset_epoch=reset_epoch,
                           reset_index=reset_index, n_miners=n_miners, n_epochs=n_epochs, resumed=resumed)
    key = (variant, reset_mode, reset_epoch, reset_index, n_miners, n_epochs, bool(resumed),
           config_key(config) if ckey is None else ckey)
    p = _PARAMS_CACHE.get(key)
    if p is None:
        p = make_params(variant, config, reset_mode=reset_mode, reset_epoch=reset_epoch,
                        reset_index=reset_index, n_miners=n_miners, n_epochs=n_epochs, resumed=resumed)
        if len(_PARAMS_CACHE) > 65536:
            _PARAMS_CACHE.clear()
        _PARAMS_CACHE[key] = p
    return p


class _NoTruthValue(Exception):
    """reset_bonds_epoch is a tensor / array whose `epoch == e` has no truth value."""

    def __init__(self, value):
        super().__init__()
        self.value = value


def _reset_epoch_value(reset_epoch) -> int | None:
    """The int epoch e at which the reference's `epoch == case.reset_bonds_epoch`
    (simulation_utils.py:63,70,81; epoch an int from range()) holds, or None
    when it never does: ints and bools (True == 1) as themselves, a float only
    when integral (20.0 == 20, 20.5 never), a one-element tensor or array as
    its element (`epoch == tensor(20)` is a truthy tensor), anything else
    never. Tensors and arrays of any other size have no truth value: the
    caller raises the reference's own error when the statement is reached."""
    if isinstance(reset_epoch, (torch.Tensor, np.ndarray)):
        n = reset_epoch.numel() if isinstance(reset_epoch, torch.Tensor) else reset_epoch.size
        if n != 1:
            raise _NoTruthValue(reset_epoch)
        return _reset_epoch_value(reset_epoch.item())
    if isinstance(reset_epoch, (bool, np.bool_, numbers.Integral)):
        return int(reset_epoch)
    if isinstance(reset_epoch, numbers.Real):
        f = float(reset_epoch)
        return int(f) if f.is_integer() else None
    return None


def _pack_reset(p: YumaParamsC, reset_mode: int, reset_epoch, reset_index, n_miners, n_epochs,
                resumed: bool = False) -> None:
    """The bond reset of run_simulation (simulation_utils.py:62-88) with the
    reference's Python indexing: `B_state[:, idx] = 0.0` and
    `server_consensus_weight[idx] == 0.0`, evaluated only at
    `epoch == reset_bonds_epoch` once B_state exists (epoch >= 1).

    - reset_epoch None or a non-integral number: never equal, no reset;
      epochs below 1 are never reached (B_state is None at epoch 0);
    - negative index: counts from the end (idx % M);
    - index None or True: `B_state[:, None]` / `B_state[:, True]` zeroes every
      column (Yuma 3.1); Yuma 3.2/4 also evaluate `scw[idx] == 0.0`, a [1, M]
      tensor whose truth value raises RuntimeError for M > 1 (for M == 1 it is
      column 0);
    - index False: `B_state[:, False]` selects nothing (Yuma 3.1: no reset);
      Yuma 3.2/4's `scw[False] == 0.0` is an empty tensor whose truth value
      raises RuntimeError;
    - index outside [-M, M): IndexError.
    The errors are raised only when the reference would reach the statement
    (reset_epoch in [1, n_epochs)). n_miners is needed for anything but a
    plain in-range non-negative index.

    resumed: the run is given a B_init, so B_state exists at epoch 0 and the
    statement is reached there too (reset_epoch in [0, n_epochs)). The
    unconditional reset (Yuma 3.1) then zeroes the caller's state before epoch
    0; the conditional ones read the previous epoch's consensus, which a run
    does not have at epoch 0, and do not fire (the kernels test t >= 1)."""
    p.reset_mode = RESET_NONE
    p.reset_epoch = -1
    p.reset_index = 0
    if reset_mode == RESET_NONE or reset_epoch is None:
        return
    try:
        epoch = _reset_epoch_value(reset_epoch)
    except _NoTruthValue as e:
        if n_epochs is None or n_epochs >= 2 or resumed:  # reached at epoch 1 (0): the reference's own error
            bool(1 == e.value)
        return
    if epoch is None or epoch < (0 if resumed else 1) or (n_epochs is not None and epoch >= n_epochs):
        return  # the statement never runs
    if not -2**31 <= epoch < 2**31:
        return  # beyond any int32 epoch count: never equal
    if isinstance(reset_index, (bool, np.bool_)) and not reset_index:
        if reset_mode == RESET_IF_ZERO_CONSENSUS:
            raise RuntimeError("Boolean value of Tensor with no values is ambiguous "
                               "(server_consensus_weight[False] == 0.0, simulation_utils.py:72,83)")
        return  # B_state[:, False] = 0.0 touches nothing
    if reset_index is None or isinstance(reset_index, (bool, np.bool_)):
        if n_miners is None:
            raise ValueError("a reset with reset_bonds_index None needs n_miners")
        if reset_mode == RESET_IF_ZERO_CONSENSUS and n_miners > 1:
            raise RuntimeError("Boolean value of Tensor with more than one value is ambiguous "
                               f"(server_consensus_weight[{reset_index}] == 0.0, simulation_utils.py:72,83)")
        if reset_mode == RESET_ALWAYS:
            p.flags |= FLAG_RESET_ALL_COLUMNS
            idx = 0
        else:
            idx = 0  # M == 1: scw[None] is the single column
    else:
        idx = operator.index(reset_index)
        if n_miners is not None:
            if not -n_miners <= idx < n_miners:
                raise IndexError(f"index {idx} is out of bounds for dimension 1 with size {n_miners}")
            idx %= n_miners
        elif idx < 0:
            raise ValueError("a negative reset_bonds_index needs n_miners to resolve")
    p.reset_mode = reset_mode
    p.reset_epoch = epoch
    p.reset_index = idx


def params_tensor(params: list[YumaParamsC], dev: torch.device) -> torch.Tensor:
    raw = b"".join(bytes(p) for p in params)
    host = torch.frombuffer(bytearray(raw), dtype=torch.uint8)
    return host.to(dev)


# ---------------------------------------------------------------------------
# engine calls
# ---------------------------------------------------------------------------
@dataclass
class RunResult:
    Dn: torch.Tensor                  # [E, N, V]
    C: torch.Tensor                   # [E, N, M]
    I: torch.Tensor                   # [E, N, M]
    B_final: torch.Tensor             # [N, V, M]
    B_hist: torch.Tensor | None       # [E, N, V, M]; [len(hist_epochs), N, V, M] under a history stride
    extra: dict
    hist_epochs: tuple[int, ...] | None = None  # the epoch each B_hist / B_watch slice holds (None: neither)
    B_watch: torch.Tensor | None = None         # [len(hist_epochs), N, V, len(watch_cols)] (run(watch=))
    watch_cols: tuple[int, ...] | None = None   # the miner column of each B_watch column
    B_move: torch.Tensor | None = None          # [E, N, 2]: max |B_t - B_{t-1}|, max |B_t| (run(want_move=True))
    B_rows: torch.Tensor | None = None          # [len(hist_epochs), N, len(watch_rows), M] (run(watch_rows=))
    watch_rows: tuple[int, ...] | None = None   # the validator row of each B_rows row
    # [E, N, V, 3]: per validator max |B_t - B_{t-1}|, max |B_t|, sum B_t (run(want_row_stats=True))
    B_rowstat: torch.Tensor | None = None


def _as_dev(x: torch.Tensor, dev) -> torch.Tensor:
    return x.to(device=dev, dtype=torch.float32).contiguous()


_MATRIX_OUTPUTS = ("Wn", "Wc", "Wb", "B_inst", "Tv")  # what the uint16 path does not produce


def u16_native(variant: int, N: int, E: int, V: int, M: int, want_hist: bool = False,
               want: tuple[str, ...] = (), *, shared_inputs: bool = False) -> bool:
    """Whether `run` on a torch.uint16 W with these arguments reads the 16-bit
    weights natively (yuma_u16_native; needs the library, not a GPU): Yuma 3 /
    Yuma 4, V <= 1024, M % 4 == 0, no shared inputs, none of Wn / Wc / Wb /
    B_inst / Tv wanted. Otherwise `run` widens W to fp32 on the device."""
    names = {"Dn", "C", "I", "B_final", *want}
    if want_hist:
        names.add("B_hist")
    outs = YumaOutputsC(**{k: (1 if k in names else None) for k in OUTPUT_FIELDS})
    flags = RUN_SHARED_INPUTS if shared_inputs else 0
    return bool(load_library().yuma_u16_native(variant, N, E, V, M, ctypes.addressof(outs), flags))


def hist_bf16_native(variant: int, N: int, E: int, V: int, M: int, *, shared_inputs: bool = False,
                     want_hist: bool = True) -> bool:
    """Whether `run` with hist_dtype=torch.bfloat16 and these arguments has the
    bond scan write the history as bfloat16 (yuma_hist_bf16_native; needs the
    library, not a GPU): Yuma 3 / Yuma 4, any V, M % 4 == 0, no shared inputs,
    a history wanted. Otherwise `run` converts an fp32 history on the device
    and RunGraph refuses."""
    outs = YumaOutputsC(B_hist=1 if want_hist else None)
    flags = RUN_SHARED_INPUTS if shared_inputs else 0
    return bool(load_library().yuma_hist_bf16_native(variant, N, E, V, M, ctypes.addressof(outs), flags))


_SCHED_REFUSED = _MATRIX_OUTPUTS + ("P", "T")  # what a run under an input schedule does not produce


def sched_native(variant: int, N: int, E: int, K: int, V: int, M: int, want_hist: bool = False,
                 want: tuple[str, ...] = (), *, shared_inputs: bool = False, w_u16: bool = False,
                 hist_bf16: bool = False) -> bool:
    """Whether `run(..., sched=)` with these arguments takes the schedule
    natively (yuma_sched_native; needs the library, not a GPU): Yuma 3 / Yuma 4,
    any V, M % 4 == 0, no shared inputs, none of Wn / Wc / Wb / B_inst / Tv /
    P / T wanted; with w_u16 / hist_bf16, where u16_native / hist_bf16_native
    hold too. Otherwise `run` expands W and S on the device and RunGraph
    refuses."""
    names = {"Dn", "C", "I", "B_final", *want}
    if want_hist:
        names.add("B_hist")
    outs = YumaOutputsC(**{k: (1 if k in names else None) for k in OUTPUT_FIELDS})
    flags = ((RUN_SHARED_INPUTS if shared_inputs else 0) | (RUN_W_U16 if w_u16 else 0)
             | (RUN_HIST_BF16 if hist_bf16 else 0))
    return bool(load_library().yuma_sched_native(variant, N, E, K, V, M, ctypes.addressof(outs), flags))


def watch_native(variant: int, N: int, E: int, V: int, M: int, n_watch: int, *, shared_inputs: bool = False,
                 w_u16: bool = False) -> bool:
    """Whether `run(..., watch=)` with these arguments has the engine write the
    watched history itself (yuma_watch_native; needs the library, not a GPU):
    Yuma 3 / Yuma 4, any V, any M and alignment, no shared inputs. Otherwise
    `run` writes an fp32 history and gathers the columns, and RunGraph refuses."""
    flags = (RUN_SHARED_INPUTS if shared_inputs else 0) | (RUN_W_U16 if w_u16 else 0)
    return bool(load_library().yuma_watch_native(variant, N, E, V, M, n_watch, flags))


def rows_native(variant: int, N: int, E: int, V: int, M: int, n_rows: int, *, shared_inputs: bool = False,
                w_u16: bool = False) -> bool:
    """Whether `run(..., watch_rows=)` with these arguments has the engine write
    the watched rows' history itself (yuma_rows_native; needs the library, not a
    GPU): Yuma 3 / Yuma 4, any V, any M and alignment, no shared inputs; with
    w_u16, where u16_native holds too. Otherwise `run` writes an fp32 history
    and gathers the rows, and RunGraph refuses."""
    flags = (RUN_SHARED_INPUTS if shared_inputs else 0) | (RUN_W_U16 if w_u16 else 0)
    return bool(load_library().yuma_rows_native(variant, N, E, V, M, n_rows, flags))


def move_native(variant: int, N: int, E: int, V: int, M: int, want_hist: bool = False,
                want: tuple[str, ...] = (), *, shared_inputs: bool = False, w_u16: bool = False) -> bool:
    """Whether `run(..., want_move=True)` with these arguments has the bond scan
    form B_move itself (yuma_move_native; needs the library, not a GPU): Yuma 3
    / Yuma 4, any V, M % 4 == 0, no shared inputs, no history and none of Wn /
    Wc / Wb / B_inst / Tv wanted; with w_u16, where u16_native holds too.
    Otherwise `run` reduces a dense fp32 history and RunGraph refuses."""
    names = {"Dn", "C", "I", "B_final", *want}
    if want_hist:
        names.add("B_hist")
    outs = YumaOutputsC(**{k: (1 if k in names else None) for k in OUTPUT_FIELDS})
    flags = (RUN_SHARED_INPUTS if shared_inputs else 0) | (RUN_W_U16 if w_u16 else 0)
    return bool(load_library().yuma_move_native(variant, N, E, V, M, ctypes.addressof(outs), flags))


def rowstat_native(variant: int, N: int, E: int, V: int, M: int, want_hist: bool = False,
                   want: tuple[str, ...] = (), *, shared_inputs: bool = False, w_u16: bool = False) -> bool:
    """Whether `run(..., want_row_stats=True)` with these arguments has the bond
    scan form B_rowstat itself (yuma_rowstat_native; needs the library, not a
    GPU): Yuma 3 / Yuma 4, any V, M % 4 == 0, fp32 weights, no shared inputs, no
    history and none of Wn / Wc / Wb / B_inst / Tv wanted. Otherwise `run`
    reduces a dense fp32 history and RunGraph refuses."""
    names = {"Dn", "C", "I", "B_final", *want}
    if want_hist:
        names.add("B_hist")
    outs = YumaOutputsC(**{k: (1 if k in names else None) for k in OUTPUT_FIELDS})
    flags = (RUN_SHARED_INPUTS if shared_inputs else 0) | (RUN_W_U16 if w_u16 else 0)
    return bool(load_library().yuma_rowstat_native(variant, N, E, V, M, ctypes.addressof(outs), flags))


def workspace_bytes_rowstat(variant: int, N: int, E: int, V: int, M: int, full_outputs: bool = False) -> int:
    """Workspace bytes of a run with the row summary (yuma_workspace_bytes_rowstat):
    the run's own and a second array of quad partials for the row totals."""
    return int(load_library().yuma_workspace_bytes_rowstat(variant, N, E, V, M, 1 if full_outputs else 0))


def resets_native(variant: int, N: int, E: int, V: int, M: int, want_hist: bool = False,
                  want: tuple[str, ...] = (), *, shared_inputs: bool = False, w_u16: bool = False,
                  hist_bf16: bool = False) -> bool:
    """Whether `run(..., resets=)` with these arguments applies the events
    inside its bond scan (yuma_resets_native; needs the library, not a GPU):
    Yuma 3 / Yuma 4, any V, M % 4 == 0, fp32 weights, no shared inputs, an fp32
    history or none, none of Wn / Wc / Wb / B_inst / Tv wanted. Otherwise `run`
    cuts the run at the event epochs and RunGraph refuses."""
    names = {"Dn", "C", "I", "B_final", *want}
    if want_hist:
        names.add("B_hist")
    outs = YumaOutputsC(**{k: (1 if k in names else None) for k in OUTPUT_FIELDS})
    flags = ((RUN_SHARED_INPUTS if shared_inputs else 0) | (RUN_W_U16 if w_u16 else 0)
             | (RUN_HIST_BF16 if hist_bf16 else 0))
    return bool(load_library().yuma_resets_native(variant, N, E, V, M, ctypes.addressof(outs), flags))


def events_native(variant: int, N: int, E: int, V: int, M: int, want_hist: bool = False,
                  want: tuple[str, ...] = (), *, shared_inputs: bool = False, w_u16: bool = False,
                  hist_bf16: bool = False) -> bool:
    """Whether `run(..., row_resets=)` with these arguments applies the row
    events inside its bond scan (yuma_events_native; needs the library, not a
    GPU): the set of resets_native. Otherwise `run` cuts the run at the event
    epochs and RunGraph refuses."""
    names = {"Dn", "C", "I", "B_final", *want}
    if want_hist:
        names.add("B_hist")
    outs = YumaOutputsC(**{k: (1 if k in names else None) for k in OUTPUT_FIELDS})
    flags = ((RUN_SHARED_INPUTS if shared_inputs else 0) | (RUN_W_U16 if w_u16 else 0)
             | (RUN_HIST_BF16 if hist_bf16 else 0))
    return bool(load_library().yuma_events_native(variant, N, E, V, M, ctypes.addressof(outs), flags))


def workspace_bytes_events(variant: int, N: int, E: int, V: int, M: int, full_outputs: bool = False) -> int:
    """yuma_workspace_bytes_events: the workspace of a run with row events (the
    reset-event workspace and the row table, one 32-bit word per epoch,
    scenario and validator)."""
    return int(load_library().yuma_workspace_bytes_events(variant, N, E, V, M, 1 if full_outputs else 0))


def _row_resets_host(row_resets, N: int, E: int, V: int) -> torch.Tensor:
    """A host row-event list as a CPU int64 tensor [n, 4] of (epoch, scenario,
    validator, 0), validated: integers, shape [n, 3] or [n, 4], epoch in
    [0, E), scenario in [0, N), validator in [0, V), the fourth (reserved)
    field 0. ValueError otherwise."""
    t = row_resets if isinstance(row_resets, torch.Tensor) else torch.as_tensor(np.asarray(row_resets))
    if t.numel() == 0:
        return torch.zeros((0, 4), dtype=torch.int64)
    if t.dtype.is_floating_point or t.dtype.is_complex or t.dtype == torch.bool:
        raise ValueError(f"row_resets must hold integers, not {t.dtype}")
    if t.dim() != 2 or t.shape[1] not in (3, 4):
        raise ValueError(f"row_resets must be (epoch, scenario, validator) events, shape [n, 3] or [n, 4], "
                         f"not {tuple(t.shape)}")
    h = t.detach().to(device="cpu", dtype=torch.int64)
    if h.shape[1] == 3:
        h = torch.cat([h, torch.zeros((h.shape[0], 1), dtype=torch.int64)], dim=1)
    for j, (name, lo, hi) in enumerate((("epoch", 0, E), ("scenario", 0, N), ("validator", 0, V), ("reserved", 0, 1))):
        bad = (h[:, j] < lo) | (h[:, j] >= hi)
        if bool(bad.any()):
            k = int(bad.nonzero()[0])
            raise ValueError(f"row_resets[{k}]: {name} {int(h[k, j])} is outside [{lo}, {hi})")
    return h


def _resets_host(resets, N: int, E: int, M: int) -> torch.Tensor:
    """A host event list as a CPU int64 tensor [n, 4] of (epoch, scenario,
    column, mode), validated: integers, epoch in [0, E), scenario in [0, N),
    column in [-1, M) (-1: every column), mode RESET_ALWAYS or
    RESET_IF_ZERO_CONSENSUS. ValueError otherwise."""
    t = resets if isinstance(resets, torch.Tensor) else torch.as_tensor(np.asarray(resets))
    if t.numel() == 0:
        return torch.zeros((0, 4), dtype=torch.int64)
    if t.dtype.is_floating_point or t.dtype.is_complex or t.dtype == torch.bool:
        raise ValueError(f"resets must hold integers, not {t.dtype}")
    if t.dim() != 2 or t.shape[1] != 4:
        raise ValueError(f"resets must be (epoch, scenario, column, mode) events, shape [n, 4], not {tuple(t.shape)}")
    h = t.detach().to(device="cpu", dtype=torch.int64)
    for j, (name, lo, hi) in enumerate((("epoch", 0, E), ("scenario", 0, N), ("column", -1, M))):
        bad = (h[:, j] < lo) | (h[:, j] >= hi)
        if bool(bad.any()):
            k = int(bad.nonzero()[0])
            raise ValueError(f"resets[{k}]: {name} {int(h[k, j])} is outside [{lo}, {hi})")
    bad = (h[:, 3] != RESET_ALWAYS) & (h[:, 3] != RESET_IF_ZERO_CONSENSUS)
    if bool(bad.any()):
        k = int(bad.nonzero()[0])
        raise ValueError(f"resets[{k}]: mode {int(h[k, 3])} is neither RESET_ALWAYS nor RESET_IF_ZERO_CONSENSUS")
    return h


def _run_segments(variant, params, W, S, B_init, Wprev_init, ev, *, N, E, M, h_epochs, want_hist, want,
                  chunk_epochs, workspace, out, shared_inputs, hist_stride, row_ev=None) -> "RunResult":
    """run(..., resets=) where the events are not native: the chain that defines
    them. The run is cut at the distinct event epochs; each segment runs on the
    existing path from the carried B_final, whose columns torch zeroes between
    segments (conditional events read the previous segment's last C); the
    params' own reset is folded into the event list and cleared in copied
    records; the history's phase is carried from segment to segment; per-epoch
    outputs and history slots are concatenated. ev: CPU int64 [n, 4]; events
    the device code would ignore are dropped here. row_ev: the row events
    (run(..., row_resets=)), CPU int64 [n, 4] of (epoch, scenario, validator,
    reserved) or None: the run is cut at their epochs too and the rows are
    zeroed beside the columns."""
    dev = device()
    ok = ((ev[:, 0] >= 0) & (ev[:, 0] < E) & (ev[:, 1] >= 0) & (ev[:, 1] < N) & (ev[:, 2] >= -1) & (ev[:, 2] < M)
          & ((ev[:, 3] == RESET_ALWAYS) | ((ev[:, 3] == RESET_IF_ZERO_CONSENSUS) & (ev[:, 2] >= 0) & (ev[:, 0] >= 1))))
    events = [tuple(int(x) for x in row) for row in ev[ok].tolist()]
    prm = []
    for n, p in enumerate(params):
        q = YumaParamsC.from_buffer_copy(bytes(p))
        if q.reset_mode != RESET_NONE and 0 <= q.reset_epoch < E:
            all_cols = bool(q.flags & FLAG_RESET_ALL_COLUMNS)
            if all_cols or 0 <= q.reset_index < M:
                if q.reset_mode == RESET_ALWAYS or (not all_cols and q.reset_epoch >= 1):
                    events.append((q.reset_epoch, n, -1 if all_cols else q.reset_index, q.reset_mode))
        q.reset_mode, q.reset_epoch, q.reset_index = RESET_NONE, -1, 0
        q.flags &= ~FLAG_RESET_ALL_COLUMNS
        prm.append(q)
    by_epoch: dict = {}
    for t, n, c, mode in events:
        by_epoch.setdefault(t, []).append((n, c, mode))
    rows_by_epoch: dict = {}
    if row_ev is not None:
        V_ = W.shape[2]
        for t, n, v, z in row_ev.tolist():
            if 0 <= t < E and 0 <= n < N and 0 <= v < V_ and z == 0:
                rows_by_epoch.setdefault(t, []).append((n, v))
                by_epoch.setdefault(t, [])
    cuts = [0] + sorted(t for t in by_epoch if t > 0) + [E]

    def apply(B, evs, prevC, rows=()):
        """B [N, V, M] with the columns of the events evs and the rows (n, v) zeroed (prevC [N, M]: C of the epoch
        before)."""
        if rows:
            B = B.clone()
            for n, v in rows:
                B[n, v, :] = 0.0
        mask = torch.zeros((N, M), dtype=torch.bool, device=dev)
        for n, c, mode in evs:
            if mode == RESET_ALWAYS:
                if c < 0:
                    mask[n, :] = True
                else:
                    mask[n, c] = True
            elif prevC is not None:
                mask[n, c] |= prevC[n, c] == 0.0
        return B.masked_fill(mask[:, None, :], 0.0)

    B = None if B_init is None else _as_dev(B_init, dev)
    if B is not None and 0 in by_epoch:
        B = apply(B, by_epoch[0], None, rows_by_epoch.get(0, ()))
    parts, hist, last = [], [], None
    names = ("Dn", "C", "I") + tuple(want)
    for a, b in zip(cuts[:-1], cuts[1:]):
        if a > 0:
            B = apply(last.B_final, by_epoch[a], last.C[-1], rows_by_epoch.get(a, ()))
        stored = [t for t in h_epochs if a <= t < b] if want_hist else []
        last = run(variant, prm, W[a:b], S[a:b], B, Wprev_init if a == 0 else None, want_hist=bool(stored), want=want,
                   chunk_epochs=chunk_epochs, workspace=workspace, shared_inputs=shared_inputs,
                   hist_stride=hist_stride if stored else 1, hist_first=stored[0] - a if stored else None)
        parts.append({k: (getattr(last, k) if k in ("Dn", "C", "I") else last.extra[k]) for k in names})
        if stored:
            hist.append(last.B_hist)
    res = {k: torch.cat([p[k] for p in parts]) for k in names}
    res["B_final"] = last.B_final
    V = last.B_final.shape[1]
    if want_hist:
        res["B_hist"] = torch.cat(hist) if hist else torch.empty((0, N, V, M), dtype=torch.float32, device=dev)
    for k, t in (out or {}).items():  # a caller's buffers receive the chain's results
        if t is not None and k in res:
            res[k] = t.copy_(res[k])
    extra = {k: res[k] for k in want}
    extra.update(resets_path="segments", resets=None, w_path=last.extra["w_path"], hist_path="f32")
    if row_ev is not None:
        extra["row_resets"] = None
    return RunResult(res["Dn"], res["C"], res["I"], res["B_final"], res.get("B_hist"), extra,
                     h_epochs if want_hist else None)


def move_from_history(hist: torch.Tensor, B_init: torch.Tensor | None) -> torch.Tensor:
    """B_move [E, N, 2] of a dense fp32 history [E, N, V, M], by the two
    expressions that define it: (hist[t] - hist[t-1]).abs().amax((-2, -1)) and
    hist[t].abs().amax((-2, -1)), hist[-1] being B_init or zeros. A block of
    epochs at a time, so that the temporaries stay small beside the history."""
    E, N, V, M = hist.shape
    out = torch.empty((E, N, 2), dtype=torch.float32, device=hist.device)
    first = torch.zeros((1, N, V, M), dtype=torch.float32, device=hist.device) if B_init is None else B_init[None]
    step = max(1, (1 << 26) // max(1, N * V * M))
    for t0 in range(0, E, step):
        cur = hist[t0:t0 + step]
        prev = torch.cat([first if t0 == 0 else hist[t0 - 1:t0], cur[:-1]])
        out[t0:t0 + step, :, 0] = (cur - prev).abs().amax((-2, -1))
        out[t0:t0 + step, :, 1] = cur.abs().amax((-2, -1))
    return out


def rowstat_from_history(hist: torch.Tensor, B_init: torch.Tensor | None) -> torch.Tensor:
    """B_rowstat [E, N, V, 3] of a dense fp32 history [E, N, V, M]: the two
    amax(-1) expressions that define columns 0 and 1, and the fp32 sum(-1) as
    column 2 (torch's order, not the scan's canonical one). A block of epochs at
    a time, as move_from_history."""
    E, N, V, M = hist.shape
    out = torch.empty((E, N, V, 3), dtype=torch.float32, device=hist.device)
    first = torch.zeros((1, N, V, M), dtype=torch.float32, device=hist.device) if B_init is None else B_init[None]
    step = max(1, (1 << 26) // max(1, N * V * M))
    for t0 in range(0, E, step):
        cur = hist[t0:t0 + step]
        prev = torch.cat([first if t0 == 0 else hist[t0 - 1:t0], cur[:-1]])
        out[t0:t0 + step, :, :, 0] = (cur - prev).abs().amax(-1)
        out[t0:t0 + step, :, :, 1] = cur.abs().amax(-1)
        out[t0:t0 + step, :, :, 2] = cur.sum(-1)
    return out


def settled_epoch_rows(B_rowstat, tol: float, *, relative: bool = False) -> torch.Tensor:
    """When each validator's bonds stopped moving: settled_epoch for rows.
    B_rowstat is [E, ..., V, 3] (a RunResult's [E, N, V, 3], or one scenario's
    [E, V, 3]; torch or numpy, on any device): for every index (n, v) the first
    epoch t with B_rowstat[t', n, v, 0] <= tol for every t' >= t, or (relative)
    <= tol * B_rowstat[t', n, v, 1]. E where no such t exists; a NaN entry
    never counts as settled. Returns a CPU int64 tensor of shape
    B_rowstat.shape[1:-1], [N, V]. Pure torch: needs neither the library nor a GPU."""
    b = torch.as_tensor(B_rowstat).detach().to("cpu")
    if b.dim() < 3 or b.shape[-1] != 3:
        raise ValueError(f"B_rowstat shape {tuple(b.shape)} is not [E, ..., V, 3]")
    return settled_epoch(b[..., :2], tol, relative=relative)


def settled_epoch(B_move, tol: float, *, relative: bool = False) -> torch.Tensor:
    """When the bonds stopped moving. B_move is [E, ..., 2] (a RunResult's
    [E, N, 2], or one run's [E, 2]; torch or numpy, on any device): for every
    leading index n the first epoch t with B_move[t', n, 0] <= tol for every
    t' >= t, or (relative) B_move[t', n, 0] <= tol * B_move[t', n, 1] -- the
    form Yuma 3 needs, whose bonds carry the 2^64 maxint scale. E where no such
    t exists; a NaN entry never counts as settled. Returns a CPU int64 tensor
    of shape B_move.shape[1:-1]. Pure torch: needs neither the library nor a
    GPU."""
    b = torch.as_tensor(B_move).detach().to("cpu")
    if b.dim() < 2 or b.shape[-1] != 2:
        raise ValueError(f"B_move shape {tuple(b.shape)} is not [E, ..., 2]")
    moved, size = b[..., 0], b[..., 1]
    ok = moved <= (tol * size if relative else tol)  # (a NaN on either side compares false)
    E = b.shape[0]
    idx = torch.arange(E, dtype=torch.int64).reshape((E,) + (1,) * (ok.dim() - 1))
    last_bad = torch.where(~ok, idx, torch.full_like(idx, -1)).amax(0) if E else torch.full(ok.shape[1:], -1)
    return (last_bad + 1).to(torch.int64)


class YumaScanPlanC(ctypes.Structure):
    """yuma_scan_plan_t (include/yuma_hip.h): 80 bytes."""
    _fields_ = [("grid", ctypes.c_longlong)] + [(name, ctypes.c_int32) for name in (
        "variant", "vector_form", "w_u16", "form", "shape", "rows", "rq", "hs", "hist", "nt", "hist_bf16", "sc",
        "rowblocks", "cblocks", "block", "ptiles", "dpl", "rc")]


assert ctypes.sizeof(YumaScanPlanC) == 80, ctypes.sizeof(YumaScanPlanC)

SCAN_FORMS = ("k_bonds", "k_bonds_cn", "k_rust_big", "k_bonds_elem", "k_bonds_grp")  # YUMA_SCAN_*
ELEM_SHAPES = (None, "wide", "tile_hist", "tile", "flat1", "flat2")  # YUMA_ELEM_*
DP_LAYOUTS = ("TV", "VQ", "QTE")  # YUMA_DP_*


@dataclass(frozen=True)
class ScanPlan:
    """The bond scan a call reaches (yuma_scan_plan_t, names for its enums)."""
    form: str             # one of SCAN_FORMS
    shape: str | None     # k_bonds_elem's block shape, one of ELEM_SHAPES
    rows: int             # rows per lane (k_bonds: per thread)
    rq: bool              # divides by k_rowsum's screened reciprocals
    hs: bool              # the strided-history instantiation
    hist: bool            # writes a history
    nt: bool              # non-temporal history stores (k_bonds_elem)
    hist_bf16: bool       # the history's elements are bfloat16
    sc: bool              # under an input schedule
    vector_form: bool
    w_u16: bool
    rowblocks: int
    cblocks: int
    grid: int
    block: int
    ptiles: int
    dpl: str              # one of DP_LAYOUTS


def scan_plan(variant: int, N: int, E: int, V: int, M: int, want_hist: bool = False, want: tuple[str, ...] = (), *,
              shared_inputs: bool = False, hist_stride: int = 1, hist_first: int | None = None, w_u16: bool = False,
              hist_bf16: bool = False, sched: bool = False, vector_form: bool | None = None,
              shard_stage: bool = False) -> ScanPlan:
    """The bond scan that `run` with these arguments launches for its first
    chunk, or (shard_stage) stage 4 of `shard_stage` (yuma_scan_plan; needs the
    library, not a GPU). The arguments are `run`'s, with w_u16 / hist_bf16 /
    sched for what `run` takes natively from W.dtype, hist_dtype and sched=;
    vector_form None is M % 4 == 0 (aligned buffers). EngineError where the
    engine refuses the combination."""
    names = {"Dn", "C", "I", "B_final", *want}
    if want_hist:
        names.add("B_hist")
    outs = YumaOutputsC(**{k: (1 if k in names else None) for k in OUTPUT_FIELDS})
    opts = None
    if not shard_stage:
        h = hist_epochs(E, hist_stride, hist_first)
        opts = YumaRunOptionsC(flags=(RUN_SHARED_INPUTS if shared_inputs else 0) | (RUN_W_U16 if w_u16 else 0)
                               | (RUN_HIST_BF16 if hist_bf16 else 0),
                               hist_stride=min(int(hist_stride), E), hist_first=h[0] if h else E)
    p = YumaScanPlanC()
    vec = M % 4 == 0 if vector_form is None else bool(vector_form)
    _check(load_library().yuma_scan_plan(variant, N, E, V, M, ctypes.addressof(outs),
                                         None if opts is None else ctypes.addressof(opts), int(vec), int(sched),
                                         int(shard_stage), ctypes.addressof(p)), "yuma_scan_plan")
    return ScanPlan(form=SCAN_FORMS[p.form], shape=ELEM_SHAPES[p.shape], rows=p.rows, rq=bool(p.rq), hs=bool(p.hs),
                    hist=bool(p.hist), nt=bool(p.nt), hist_bf16=bool(p.hist_bf16), sc=bool(p.sc),
                    vector_form=bool(p.vector_form), w_u16=bool(p.w_u16), rowblocks=p.rowblocks, cblocks=p.cblocks,
                    grid=p.grid, block=p.block, ptiles=p.ptiles, dpl=DP_LAYOUTS[p.dpl])


def _watch_host(watch, M: int | None, name: str = "watch", what: str = "miner", dim: str = "M") -> torch.Tensor:
    """The watch list as a CPU int64 tensor, validated on the host: integers,
    one dimension, at least one column, every entry in [0, M) (M None: not
    negative). ValueError otherwise. what, dim: the words of the messages (a
    list of validator rows is checked against V)."""
    t = watch if isinstance(watch, torch.Tensor) else torch.as_tensor(np.asarray(watch))
    if t.dtype.is_floating_point or t.dtype.is_complex or t.dtype == torch.bool:
        raise ValueError(f"{name} must hold integer {what} indices, not {t.dtype}")
    if t.dim() != 1 or t.numel() < 1:
        raise ValueError(f"{name} must be a non-empty one-dimensional list of {what} indices, not shape "
                         f"{tuple(t.shape)}")
    h = t.detach().to(device="cpu", dtype=torch.int64)
    lo, hi = int(h.min()), int(h.max())
    if lo < 0 or (M is not None and hi >= M):
        raise ValueError(f"{name} entries must lie in [0, {dim}{'' if M is None else '=' + str(M)}): found "
                         f"{lo if lo < 0 else hi}")
    return h


def _int_view(t: torch.Tensor) -> torch.Tensor:
    """The elements of t as integers of the same width (bit patterns)."""
    if t.dtype.is_floating_point or t.dtype.is_complex:
        return t.view({2: torch.int16, 4: torch.int32, 8: torch.int64}[t.element_size()])
    if t.dtype == torch.uint16:
        return t.view(torch.int16)
    return t


def _take_slices(t: torch.Tensor, idx: torch.Tensor) -> torch.Tensor:
    """t[idx] along dimension 0, bit for bit, for every dtype `run` takes."""
    v = _int_view(t)
    return v.index_select(0, idx.to(device=t.device, dtype=torch.long)).view(t.dtype)


def dedup_slices(W: torch.Tensor, S: torch.Tensor):
    """(Wk, Sk, sched) of per-epoch inputs W [E,N,V,M] and S [E,N,V]: the
    distinct slices in order of first occurrence and the int32 schedule [E]
    with W[t] == Wk[sched[t]] and S[t] == Sk[sched[t]] -- the inputs of
    `run(..., sched=)`. Two epochs share a slice when both W[t] and S[t] are
    equal bit for bit (integer views: -0.0 and +0.0 differ, NaN payloads
    count). CPU or device tensors; W fp32 or uint16 (any dtype of 2, 4 or 8
    bytes)."""
    if W.dim() != 4 or S.dim() != 3 or tuple(S.shape) != tuple(W.shape[:3]):
        raise ValueError(f"dedup_slices takes W [E,N,V,M] and S [E,N,V], not {tuple(W.shape)} and {tuple(S.shape)}")
    E = W.shape[0]
    if E == 0:
        raise ValueError("dedup_slices needs at least one epoch")
    S = S.to(W.device)
    # classes of W rows and of S rows, then of the pairs
    _, iw = torch.unique(_int_view(W.contiguous()).reshape(E, -1), dim=0, return_inverse=True)
    _, i_s = torch.unique(_int_view(S.contiguous()).reshape(E, -1), dim=0, return_inverse=True)
    _, inv = torch.unique(iw * (int(i_s.max()) + 1) + i_s, return_inverse=True)
    K = int(inv.max()) + 1
    t = torch.arange(E, device=inv.device)
    first = torch.full((K,), E, dtype=torch.long, device=inv.device).scatter_reduce(0, inv, t, "amin")
    order = torch.argsort(first)  # classes by first occurrence
    rank = torch.empty_like(order)
    rank[order] = torch.arange(K, device=inv.device)
    reps = first[order]
    return _take_slices(W, reps), _take_slices(S, reps), rank[inv].to(torch.int32)


def _sched_host(sched, K: int) -> torch.Tensor:
    """The schedule as a CPU int64 tensor, validated on the host: integers, one
    dimension, at least one epoch, every entry in [0, K). ValueError otherwise."""
    t = sched if isinstance(sched, torch.Tensor) else torch.as_tensor(np.asarray(sched))
    if t.dtype.is_floating_point or t.dtype.is_complex or t.dtype == torch.bool:
        raise ValueError(f"sched must hold integers, not {t.dtype}")
    if t.dim() != 1 or t.numel() < 1:
        raise ValueError(f"sched must be one-dimensional with one entry per epoch, not shape {tuple(t.shape)}")
    h = t.detach().to(device="cpu", dtype=torch.int64)
    lo, hi = int(h.min()), int(h.max())
    if lo < 0 or hi >= K:
        raise ValueError(f"sched entries must lie in [0, K={K}): found {lo if lo < 0 else hi}")
    return h


def workspace_bytes_sched(variant: int, N: int, E: int, K: int, V: int, M: int, full: bool) -> int:
    return int(load_library().yuma_workspace_bytes_sched(variant, N, E, K, V, M, 1 if full else 0))


def to_u16(W: torch.Tensor) -> torch.Tensor:
    """The on-chain max-upscale of float weights to 16 bits: per row (last
    dimension) round_half_even(w / rowmax * 65535), computed in float64; an
    all-zero row stays zero. Negative, NaN or infinite entries raise
    ValueError. Returns torch.uint16 of the same shape.

    This CHANGES the weights: a row is rescaled and every entry rounded to one
    of 65536 levels, so a run on the result differs from a run on the float
    input (the normalised weights move by up to 2^-17 relative to the row
    maximum). It is the format conversion the chain applies, not a
    parity-preserving one; only a tensor that already holds integers in
    [0, 65535] with 65535 in every nonzero row maps to itself."""
    w = torch.as_tensor(W).detach().to(device="cpu", dtype=torch.float64)
    if not bool(torch.isfinite(w).all()) or bool((w < 0).any()):
        raise ValueError("to_u16 takes finite, non-negative weights")
    mx = w.amax(dim=-1, keepdim=True)
    # (w * 65535) / rowmax: the product is exact for 16-bit inputs, so a true
    # tie reaches the rounding as a tie; an all-zero row divides by 1
    q = w * 65535.0 / torch.where(mx > 0, mx, torch.ones_like(mx))
    return torch.from_numpy(np.rint(q.numpy()).astype(np.uint16))  # rint: half to even


def _as_u16(x: torch.Tensor) -> torch.Tensor:
    """Integers in [0, 65535] of any integer dtype as torch.uint16 (torch has
    no arithmetic on uint16: the value's low 16 bits through int16)."""
    x = x.to(torch.int64)
    return ((x + 32768) % 65536 - 32768).to(torch.int16).view(torch.uint16)


def pairs_from_dense(W: torch.Tensor):
    """(row_ptr int64 [rows + 1], uid uint16 [nnz], val uint16 [nnz]): the
    nonzeros of a uint16 tensor whose last dimension is M, rows (every leading
    dimension flattened) in order and each row's columns ascending -- the CSR
    pair lists yuma_weights_from_pairs takes, on W's device. The inverse of
    weights_from_pairs on lists without zero weights, dropped uids or
    duplicates. M > 65536 raises ValueError: a uid would not fit 16 bits."""
    if not isinstance(W, torch.Tensor) or W.dtype != torch.uint16 or W.dim() < 1:
        raise ValueError("pairs_from_dense takes a torch.uint16 tensor of at least one dimension")
    M = W.shape[-1]
    if M < 1 or M > 65536:
        raise ValueError(f"M={M} must lie in [1, 65536]: a uid beyond that would not fit 16 bits")
    w = W.contiguous().view(torch.int16).reshape(-1, M)
    nz = w != 0
    row_ptr = torch.zeros(w.shape[0] + 1, dtype=torch.int64, device=W.device)
    torch.cumsum(nz.sum(dim=1), dim=0, out=row_ptr[1:])
    idx = nz.nonzero()  # row-major: rows in order, columns ascending
    return row_ptr, _as_u16(idx[:, 1]), w[nz].view(torch.uint16)


@dataclass(frozen=True)
class PairsStatus:
    """The status words of one weights_from_pairs call (include/yuma_hip.h)."""
    dropped: int        # pairs with uid >= M
    conflict_rows: int  # rows holding one uid with two different weights
    bad_rows: int       # rows whose row_ptr range had to be clamped

    @classmethod
    def from_tensor(cls, status: torch.Tensor) -> "PairsStatus":
        """Reads the device words: the one place that synchronises."""
        h = [int(x) & 0xFFFFFFFF for x in status.detach().cpu().tolist()]
        return cls(dropped=h[PAIRS_ST_DROPPED], conflict_rows=h[PAIRS_ST_CONFLICT_ROWS],
                   bad_rows=h[PAIRS_ST_BAD_ROWS])


def weights_from_pairs(row_ptr: torch.Tensor, uid: torch.Tensor, val: torch.Tensor, shape, *,
                       upscale: bool = False, out: torch.Tensor | None = None, want_status: bool = True,
                       stream: "torch.cuda.Stream | None" = None):
    """The dense torch.uint16 W of the chain's (uid, weight) pair lists, built
    on the device (yuma_weights_from_pairs): (W, status).

    row_ptr int64 [rows + 1], uid and val uint16 [nnz], CPU or device: row r
    (of `shape`'s leading dimensions flattened; (E, N, V, M) for a run) owns the
    pairs [row_ptr[r], row_ptr[r + 1]). shape's last dimension is M. upscale:
    the chain's per-row max-upscale, the bits of to_u16 on the densified row.
    out: a contiguous device torch.uint16 tensor of that shape to fill (any
    2-byte alignment). status: a device int32[4] tensor for
    PairsStatus.from_tensor (dropped pairs, rows with conflicting duplicates,
    rows with a clamped range), or None with want_status=False, which also
    skips the read-back pass. stream: a torch.cuda.Stream, default the current
    one. Nothing here synchronises; what cannot be checked without reading the
    lists (row_ptr's values) is clamped on the device and reported in status.
    Dtypes, dimensions and lengths raise ValueError before the library is
    touched."""
    for name, t, dt in (("row_ptr", row_ptr, torch.int64), ("uid", uid, torch.uint16), ("val", val, torch.uint16)):
        if not isinstance(t, torch.Tensor) or t.dtype != dt or t.dim() != 1:
            raise ValueError(f"{name} must be a one-dimensional {dt} tensor, not "
                             f"{(t.dtype, tuple(t.shape)) if isinstance(t, torch.Tensor) else type(t).__name__}")
    try:
        shape = tuple(operator.index(s) for s in shape)
    except TypeError as e:
        raise ValueError(f"shape must be a sequence of integers: {e}") from e
    if not shape or min(shape) < 0 or shape[-1] < 1:
        raise ValueError(f"shape {shape} must be non-negative sizes ending in M >= 1")
    M, rows = shape[-1], math.prod(shape[:-1])
    if row_ptr.numel() != rows + 1:
        raise ValueError(f"row_ptr holds {row_ptr.numel()} entries; shape {shape} has {rows} rows and needs {rows + 1}")
    if uid.numel() != val.numel():
        raise ValueError(f"uid holds {uid.numel()} entries and val {val.numel()}")
    if out is not None and (not isinstance(out, torch.Tensor) or out.dtype != torch.uint16
                            or tuple(out.shape) != shape or not out.is_contiguous() or not out.is_cuda):
        raise ValueError(f"out must be a contiguous device torch.uint16 tensor of shape {shape}")
    if stream is not None and not isinstance(stream, torch.cuda.Stream):
        raise ValueError(f"stream must be a torch.cuda.Stream, not {type(stream).__name__}")
    dev = device()
    lib = load_library()
    if not hasattr(lib, "yuma_weights_from_pairs"):
        raise EngineError("this libyuma_hip.so lacks yuma_weights_from_pairs")
    with torch.cuda.stream(stream if stream is not None else torch.cuda.current_stream(dev)):
        rp, u, v = (t.detach().to(dev).contiguous() for t in (row_ptr, uid, val))
        W = out if out is not None else torch.empty(shape, dtype=torch.uint16, device=dev)
        # (rows == 0 launches nothing: the words are zero from the start)
        status = (torch.zeros if rows == 0 else torch.empty)(PAIRS_ST_WORDS, dtype=torch.int32, device=dev) \
            if want_status else None
        _check(lib.yuma_weights_from_pairs(rows, M, u.numel(), rp.data_ptr(), u.data_ptr(), v.data_ptr(),
                                           PAIRS_UPSCALE if upscale else 0, W.data_ptr(), _ptr(status),
                                           torch.cuda.current_stream(dev).cuda_stream), "yuma_weights_from_pairs")
    return W, status


def hist_epochs(E: int, stride: int = 1, first: int | None = None) -> tuple[int, ...]:
    """The epochs whose bond state a run of E epochs stores under a history
    stride: first, first + stride, ... below E. first=None is stride - 1, the
    state after every stride-th epoch. Host only (needs the library, not a
    GPU): the count is cross-checked against yuma_hist_slots."""
    E, stride = operator.index(E), operator.index(stride)
    if E < 1:
        raise ValueError(f"E={E} must be positive")
    if stride < 1:
        raise ValueError(f"hist_stride={stride} must be at least 1")
    first = stride - 1 if first is None else operator.index(first)
    if first < 0:
        raise ValueError(f"hist_first={first} must not be negative")
    epochs = tuple(range(first, E, stride))
    if max(E, stride, first) < 2**31:  # (beyond int32 the C entry point cannot be asked)
        n = int(load_library().yuma_hist_slots(E, stride, first))
        if n != len(epochs):
            raise EngineError(f"yuma_hist_slots({E}, {stride}, {first}) = {n}, expected {len(epochs)}")
    return epochs


def workspace_bytes(variant: int, N: int, E: int, V: int, M: int, full: bool) -> int:
    return int(load_library().yuma_workspace_bytes(variant, N, E, V, M, 1 if full else 0))


def _vector_form(W: torch.Tensor, w_u16: bool, B_init, Wprev_init, o: dict, hist_bf16: bool) -> bool:
    """The scan's vector form as the engine tests it (vector_form of the engine
    source): W on its vector alignment (16 bytes, 8 as uint16), every fp32
    matrix read or written 16-byte aligned, a bfloat16 history 8-byte. A view
    at an odd offset sends an fp32 run to the scalar scan, which the uint16,
    bfloat16-history and schedule kernels lack."""
    hist = o.get("B_hist")
    if hist is not None and hist.data_ptr() % (8 if hist_bf16 else 16):
        return False
    mats = [B_init, Wprev_init] + [o.get(k) for k in ("Wn", "Wc", "Wb", "B_inst", "B_final")]
    return W.data_ptr() % (8 if w_u16 else 16) == 0 and all(t is None or t.data_ptr() % 16 == 0 for t in mats)


def _check_args(params, W, S, B_init, Wprev_init, out, *, single_call, shared_inputs, hist_stride, hist_first,
                hist_dtype, sched, watch=None, want_move=False, want_row_stats=False):
    """run's argument checks, in the order run has always raised them: the
    history type and the schedule before anything touches a GPU, the rest
    behind device(). Returns (dev, N, E, K, sched_host, h_epochs, watch_host);
    K and sched_host are None without a schedule, watch_host without a watch
    list."""
    if hist_dtype not in (None, torch.float32, torch.bfloat16):
        raise ValueError(f"hist_dtype={hist_dtype} must be None, torch.float32 or torch.bfloat16")
    if hist_dtype == torch.bfloat16 and single_call:
        raise ValueError("single_call (yuma_epoch) writes an fp32 history: no hist_dtype=torch.bfloat16")
    if not isinstance(want_move, (bool, np.bool_)):
        raise ValueError(f"want_move must be a bool, not {type(want_move).__name__}")
    if want_move and single_call:
        raise ValueError("single_call (yuma_epoch) takes no B_move: no want_move")
    if not isinstance(want_row_stats, (bool, np.bool_)):
        raise ValueError(f"want_row_stats must be a bool, not {type(want_row_stats).__name__}")
    if want_row_stats and single_call:
        raise ValueError("single_call (yuma_epoch) takes no B_rowstat: no want_row_stats")
    E, Nw, V, M = W.shape
    K = sched_host = None
    if sched is not None:  # validated before anything touches a GPU
        K = E
        sched_host = _sched_host(sched, K)
        E = sched_host.numel()
        for name, t in (out or {}).items():  # a caller's per-epoch outputs follow the schedule's length
            if t is not None and name not in ("B_hist", "B_final") and t.shape[0] != E:
                raise ValueError(f"out[{name!r}] holds {t.shape[0]} epochs, the schedule {E}")
        if S.shape != (K, Nw, V):
            raise ValueError(f"S shape {tuple(S.shape)} is not [K={K}, N={Nw}, V={V}] of W {tuple(W.shape)}")
    watch_host = None if watch is None else _watch_host(watch, M)  # before anything touches a GPU
    check_limits(V, M)
    dev = device()
    if sched is None and S.shape != (E, Nw, V):
        raise ValueError(f"S shape {tuple(S.shape)} does not match W {tuple(W.shape)}")
    N = len(params) if shared_inputs else Nw
    h_epochs = hist_epochs(E, hist_stride, hist_first)
    if len(h_epochs) != E and single_call:  # (stride 1 from epoch 0 stores all E epochs: the dense history)
        raise ValueError("single_call (yuma_epoch) keeps the dense history: no hist_stride / hist_first")
    for name, t in (("B_init", B_init), ("Wprev_init", Wprev_init)):
        # the kernels index it n * V * M + row * M + m: a smaller tensor is read past its end
        if t is not None and tuple(t.shape) != (N, V, M):
            raise ValueError(f"{name} shape {tuple(t.shape)} is not [N={N}, V={V}, M={M}]")
    if shared_inputs:
        if Nw != 1:
            raise ValueError("shared_inputs takes W [E,1,V,M] and S [E,1,V]")
        if single_call:
            raise ValueError("single_call does not take shared inputs")
    elif len(params) != N:
        raise ValueError("one parameter record per scenario is required")
    return dev, N, E, K, sched_host, h_epochs, watch_host


def _alloc_history(o: dict, dev, shape, *, want_hist: bool, h_bf16: bool, native_ok) -> bool:
    """The history decision, up to alignment: o["B_hist"] checked or allocated
    ([n_hist, N, V, M]), bfloat16 where the scan is to write it itself. Returns
    that: hist_dtype=torch.bfloat16, a history with at least one slot, and
    native_ok() (hist_bf16_native)."""
    hist_user = o.get("B_hist") if h_bf16 else None  # the caller's bfloat16 buffer
    if hist_user is not None and hist_user.dtype != torch.bfloat16:
        raise ValueError(f"out['B_hist'] is {hist_user.dtype}, hist_dtype=torch.bfloat16 needs a bfloat16 tensor")
    # (a history of no slots is a null pointer to the engine: nothing to write in either type)
    native = h_bf16 and (want_hist or hist_user is not None) and shape[0] > 0 and native_ok()
    if want_hist and o.get("B_hist") is None:
        o["B_hist"] = torch.empty(shape, dtype=torch.bfloat16 if native else torch.float32, device=dev)
    if o.get("B_hist") is not None and tuple(o["B_hist"].shape) != shape:
        # the kernels index it slot * N * V * M + ...: a smaller tensor is written past its end
        raise ValueError(f"out['B_hist'] shape {tuple(o['B_hist'].shape)} is not "
                         f"[n_hist={shape[0]}, N={shape[1]}, V={shape[2]}, M={shape[3]}]")
    return native


_OUT_SHAPES = {
    "Dn": "ENV", "C": "ENM", "I": "ENM", "B_final": "NVM",
    "D": "ENV", "R": "ENM", "P": "ENM", "T": "ENM", "Tv": "ENV", "Sn": "ENV", "bond_alpha": "ENM", "alpha_ab": "EN2",
    "Wn": "ENVM", "Wc": "ENVM", "Wb": "ENVM", "B_inst": "ENVM",
}


def _list_section(req: YumaRequestC, bit: int, names: tuple[str, str, str], arg) -> None:
    """A watch or row list section of the request: arg is None, or the int32
    device list, its history and the buffer whose address the engine gets."""
    if arg is not None:
        req.sections |= bit
        for name, value in zip(names, (arg[0].data_ptr(), arg[0].numel(), arg[2].data_ptr())):
            setattr(req, name, value)


def _events_section(req: YumaRequestC, bit: int, names: tuple[str, str], events) -> None:
    """An event section of the request: events is None or the int32 device
    list [n, 4]; an empty list is no section (the run of yuma_run_opts)."""
    if events is not None and events.shape[0] > 0:
        req.sections |= bit
        setattr(req, names[0], events.data_ptr())
        setattr(req, names[1], events.shape[0])


def _launch(lib, dev, req: YumaRequestC, *, capture, phase_ms) -> None:
    """The run's one launch: yuma_run_request, or with `capture`
    yuma_graph_create_request, the handle appended to it."""
    if capture is not None:  # RunGraph: capture instead of launching
        h = ctypes.c_void_p()
        torch.cuda.synchronize(dev)
        _check(lib.yuma_graph_create_request(ctypes.byref(h), ctypes.addressof(req)), "yuma_graph_create_request")
        capture.append(h)
        return
    # phase_ms (bench-only): per-phase device time from HIP events (blocks)
    buf = None if phase_ms is None else (ctypes.c_float * len(PHASES))()
    _check(lib.yuma_run_request(ctypes.addressof(req), torch.cuda.current_stream(dev).cuda_stream, buf),
           "yuma_run_request")
    if phase_ms is not None:
        phase_ms[:] = list(buf)


def run(variant: int, params: list[YumaParamsC], W: torch.Tensor, S: torch.Tensor,
        B_init: torch.Tensor | None = None, Wprev_init: torch.Tensor | None = None, *,
        want_hist: bool = False, want: tuple[str, ...] = (), chunk_epochs: int = 0,
        workspace: torch.Tensor | None = None, out: dict | None = None,
        phase_ms: list | None = None, capture: list | None = None,
        single_call: bool = False, shared_inputs: bool = False,
        hist_stride: int = 1, hist_first: int | None = None, hist_dtype=None, sched=None,
        watch=None, want_move: bool = False, resets=None, watch_rows=None, row_resets=None,
        want_row_stats: bool = False) -> RunResult:
    """E epochs of N scenarios. W [E,N,V,M], S [E,N,V] (raw); optional
    B_init [N,V,M] and (Yuma2) normalised Wprev_init [N,V,M].
    single_call: E == 1 through yuma_epoch (one call of a Yuma* variant,
    yumas.py:61/175/285/399/494) instead of yuma_run_opts.
    shared_inputs: W [E,1,V,M] and S [E,1,V] are one trajectory that every
    scenario (one per params record) reads — a parameter sweep over one subnet
    (YUMA_RUN_SHARED_INPUTS); results equal a run on W and S
    replicated per scenario.
    hist_stride, hist_first: with want_hist (or out["B_hist"]), store the bond
    state after the epochs hist_epochs(E, hist_stride, hist_first) only:
    B_hist is [n_hist, N, V, M], slice j bit-equal to the dense history's slice
    at RunResult.hist_epochs[j] (yuma_run_opts). hist_first=None is
    hist_stride - 1. Stride 1 from epoch 0 is the dense history.
    hist_dtype: None / torch.float32, or torch.bfloat16: B_hist is then
    bfloat16, every element RNE(fp32 bond state); every other output keeps the
    bits of the fp32-history run. Where hist_bf16_native holds (and B_hist is
    8-byte aligned) the bond scan writes the 16-bit history itself
    (YUMA_RUN_HIST_BF16, extra["hist_path"] == "bf16"); elsewhere the run
    writes an fp32 history and converts it on the device (extra["hist_path"] ==
    "f32"; a captured run raises EngineError instead). A caller's out["B_hist"]
    must be bfloat16. For reading, not for resuming: resume from B_final.
    sched: an input schedule, a sequence or integer tensor of length E. W is
    then [K,N,V,M] and S [K,N,V], the stored slices, and epoch t reads slice
    sched[t] (dedup_slices builds the three from per-epoch inputs). Every
    output, hist_epochs included, is that of the run on W[sched], S[sched],
    bit for bit. The schedule is validated on the host (ValueError). Where
    sched_native holds (and the buffers have the vector form's alignment) the
    engine stores K slices and runs phase 1 once per stored slice
    (yuma_run_sched, extra["sched_path"] == "native"; extra["sched"] is the
    int32 device tensor a captured run re-reads at every replay); elsewhere,
    and under single_call, the inputs are expanded on the device and the dense
    path runs (extra["sched_path"] == "expanded"; a captured run raises
    EngineError instead).
    watch: a non-empty sequence or integer tensor of miner indices (duplicates
    and any order allowed; validated on the host, ValueError): the result's
    B_watch [n_hist, N, V, len(watch)] is the fp32 bond history of those
    columns alone, bit-equal to B_hist[..., watch] of the run without a watch
    list, at the epochs hist_stride / hist_first select (RunResult.hist_epochs;
    watch_cols names the columns). want_hist=False with watch= is the normal
    call: the main run then takes the history-less scans; both together give
    both histories. Where watch_native holds the engine writes B_watch itself
    (yuma_run_watch, extra["watch_path"] == "native"; extra["watch"] is the
    int32 device list a captured run re-reads at every replay -- a caller's own
    contiguous int32 device tensor is used as it is); elsewhere (Yuma 0 / 1 /
    2, shared inputs, single_call) the run writes an fp32 history, the columns
    are gathered from it on the device and the dense history is dropped unless
    asked for (extra["watch_path"] == "dense"; a captured run raises
    EngineError instead).
    want_move: the result's B_move [E, N, 2] (fp32, on the device) holds per
    epoch and scenario max over (v, m) of |B_t - B_{t-1}| and of |B_t|, B_t the
    bond state after epoch t with the dense fp32 history's bits (a reset at
    epoch t is part of epoch t's movement; B_{-1} is B_init or zeros): bit-equal
    to (hist[t] - hist[t-1]).abs().amax((-2, -1)) and hist[t].abs().amax((-2,
    -1)) on that history, NaN as in torch.amax, independent of chunk_epochs;
    every other output keeps its bits (settled_epoch reads it). Where
    move_native holds (and the buffers have the vector form's alignment) the
    history-less scan forms it in registers (yuma_run_move, extra["move_path"]
    == "native"); elsewhere (Yuma 0 / 1 / 2, shared inputs, the scalar form, a
    history requested in the same run) the run writes a dense fp32 history,
    B_move is reduced from it on the device, a requested strided and / or
    bfloat16 history is taken from it, and it is dropped unless asked for
    (extra["move_path"] == "dense"; a captured run raises EngineError
    instead).
    resets: bond reset events, a sequence of (epoch, scenario, column, mode)
    tuples or an int32 tensor [n, 4]: before epoch t's update of scenario n the
    event zeroes bond column c (-1: every column, RESET_ALWAYS only) if a bond
    state exists (t >= 1, or B_init given) and the mode's rule holds --
    RESET_ALWAYS always, RESET_IF_ZERO_CONSENSUS iff t >= 1 and C[t-1, n, c] ==
    0. Duplicates and any order are allowed; the params' own reset keeps
    working beside the events. A host sequence (or CPU tensor) is validated
    before anything touches a GPU (ValueError); a CUDA tensor is passed through
    unchecked, and the device code ignores an event out of range. Every output
    has the bits of the chain of runs cut at the event epochs and resumed from
    B_final with the columns zeroed. Yuma 3 / Yuma 4 only, and not together
    with sched, watch, want_move, single_call or a bfloat16 history
    (ValueError). Where resets_native holds (and the buffers have the vector
    form's alignment) the bond scan applies the events itself
    (yuma_run_resets, extra["resets_path"] == "native"; extra["resets"] is the
    int32 device list a captured run re-reads at every replay -- a caller's own
    contiguous int32 device tensor is used as it is); elsewhere (the scalar
    form, shared inputs, uint16 weights, the full-output matrices) that chain
    runs (extra["resets_path"] == "segments"; a captured run raises EngineError
    instead).
    want_row_stats: the result's B_rowstat [E, N, V, 3] (fp32, on the device)
    holds per epoch, scenario and validator max over m of |B_t - B_{t-1}|, max
    over m of |B_t| and sum over m of B_t, B_t as for want_move: columns 0 and
    1 are bit-equal to (hist[t] - hist[t-1]).abs().amax(-1) and
    hist[t].abs().amax(-1) on the dense fp32 history, and their amax over v is
    B_move; every other output keeps its bits (settled_epoch_rows reads it).
    Where rowstat_native holds, W is not uint16, no history, schedule or
    want_move rides in the same run and the buffers have the vector form's
    alignment, the history-less scan forms it (yuma_run_rowstat,
    extra["rowstat_path"] == "native"): column 2 is then summed in the
    canonical order of the dividends (include/yuma_hip.h) and has the same bits
    for every chunk_epochs and scan shape. Elsewhere the run writes a dense
    fp32 history and reduces it on the device, column 2 as the fp32 sum(-1),
    and drops the history unless asked for (extra["rowstat_path"] == "dense"; a
    captured run raises EngineError instead). watch= and watch_rows= combine
    with the native path; resets= and row_resets= do not combine at all
    (ValueError).
    watch_rows: a non-empty sequence or integer tensor of validator indices
    (duplicates and any order allowed; validated on the host, ValueError): the
    result's B_rows [n_hist, N, len(watch_rows), M] is the fp32 bond history of
    those validators' rows alone, bit-equal to B_hist[:, :, watch_rows, :] of
    the run without a row list, at the epochs hist_stride / hist_first select
    (RunResult.hist_epochs; RunResult.watch_rows names the rows). Like watch=,
    it lets the main run take the history-less scans; it combines with
    hist_stride / hist_first, sched, uint16 W, watch, want_move, want_hist
    (both histories are written), B_init and chunk_epochs, and not with
    resets= (ValueError). Where rows_native holds the engine writes B_rows
    itself (yuma_run_rows, extra["rows_path"] == "native"; extra["watch_rows"]
    is the int32 device list a captured run re-reads at every replay -- a
    caller's own contiguous int32 device tensor is used as it is); elsewhere
    (Yuma 0 / 1 / 2, shared inputs, single_call) the run writes an fp32
    history, the rows are gathered from it on the device and the history is
    dropped unless asked for (extra["rows_path"] == "dense"; a captured run
    raises EngineError instead).
    row_resets: validator-row events, a sequence of (epoch, scenario,
    validator) tuples or an int32 tensor [n, 3] or [n, 4] (the fourth field is
    reserved: 0): before epoch t's update of scenario n the event zeroes bond
    row v, B[n, v, :] = 0, if a bond state exists (t >= 1, or B_init given);
    no consensus rule applies to a validator. Duplicates and any order are
    allowed; resets= and the params' own reset keep working beside the row
    events, and the two kinds commute. A host sequence (or CPU tensor) is
    validated before anything touches a GPU (ValueError); a CUDA tensor is
    passed through unchecked, and the device code ignores an event out of
    range or with a non-zero reserved field. Every output has the bits of the
    chain of runs cut at the event epochs and resumed from B_final with the
    rows and columns zeroed. It combines with resets=, want_hist, hist_stride /
    hist_first, B_init and chunk_epochs; like resets= it takes Yuma 3 / Yuma 4
    only, and not sched, watch, watch_rows, want_move, single_call or a
    bfloat16 history (ValueError). Where events_native holds (and the buffers
    have the vector form's alignment) the bond scan applies the events itself
    (yuma_run_events, extra["resets_path"] == "native"; extra["row_resets"] is
    the int32 device list [n, 4] a captured run re-reads at every replay -- a
    caller's own contiguous int32 [n, 4] device tensor is used as it is);
    elsewhere that chain runs (extra["resets_path"] == "segments"; a captured
    run raises EngineError instead)."""
    h_bf16 = hist_dtype == torch.bfloat16
    # the row list, validated before anything touches a GPU
    rows_host = None if watch_rows is None else _watch_host(watch_rows, W.shape[2], "watch_rows", "validator", "V")
    resets_host = None
    if resets is not None:  # refused and validated before anything touches a GPU
        if variant not in (VARIANT_YUMA3, VARIANT_YUMA4):
            raise ValueError("resets= takes Yuma 3 / Yuma 4 only")
        for name, given in (("sched", sched is not None), ("watch_rows", watch_rows is not None),
                            ("watch", watch is not None), ("want_move", bool(want_move)),
                            ("want_row_stats", bool(want_row_stats)),
                            ("single_call", bool(single_call)), ("hist_dtype=torch.bfloat16", h_bf16)):
            if given:
                raise ValueError(f"resets= does not combine with {name}")
        if isinstance(resets, torch.Tensor) and resets.is_cuda:
            if resets.dtype != torch.int32 or resets.dim() != 2 or resets.shape[1] != 4:
                raise ValueError(f"a device event list must be int32 [n, 4], not {resets.dtype} {tuple(resets.shape)}")
        else:
            resets_host = _resets_host(resets, len(params) if shared_inputs else W.shape[1], W.shape[0], W.shape[3])
    rowev_host = None
    if row_resets is not None:  # likewise
        if variant not in (VARIANT_YUMA3, VARIANT_YUMA4):
            raise ValueError("row_resets= takes Yuma 3 / Yuma 4 only")
        for name, given in (("sched", sched is not None), ("watch_rows", watch_rows is not None),
                            ("watch", watch is not None), ("want_move", bool(want_move)),
                            ("want_row_stats", bool(want_row_stats)),
                            ("single_call", bool(single_call)), ("hist_dtype=torch.bfloat16", h_bf16)):
            if given:
                raise ValueError(f"row_resets= does not combine with {name}")
        if isinstance(row_resets, torch.Tensor) and row_resets.is_cuda:
            if row_resets.dtype != torch.int32 or row_resets.dim() != 2 or row_resets.shape[1] not in (3, 4):
                raise ValueError(f"a device row-event list must be int32 [n, 3] or [n, 4], not {row_resets.dtype} "
                                 f"{tuple(row_resets.shape)}")
        else:
            rowev_host = _row_resets_host(row_resets, len(params) if shared_inputs else W.shape[1], W.shape[0],
                                          W.shape[2])
    dev, N, E, K, sched_host, h_epochs, watch_host = _check_args(
        params, W, S, B_init, Wprev_init, out, single_call=single_call, shared_inputs=shared_inputs,
        hist_stride=hist_stride, hist_first=hist_first, hist_dtype=hist_dtype, sched=sched, watch=watch,
        want_move=want_move, want_row_stats=want_row_stats)
    V, M = W.shape[2:]
    lib = load_library()
    W_arg, S_arg = W, S  # as given: the code below rebinds W and S (widened, moved, expanded under a schedule)

    def move_dense():
        """B_move (and / or B_rowstat) from a dense fp32 history of the same run, on the inputs and
        the schedule as the caller gave them; the history asked for (its stride,
        its type, the caller's buffer) and B_watch from it."""
        if capture is not None and want_row_stats:
            raise EngineError("a captured run cannot reduce a dense history: want_row_stats needs "
                              "rowstat_native(variant, N, E, V, M, ...), fp32 weights, no history, schedule or "
                              "want_move in the same run and vector-aligned buffers")
        if capture is not None:
            raise EngineError("a captured run cannot reduce a dense history: want_move needs "
                              "move_native(variant, N, E, V, M, ...), no history in the same run and "
                              "vector-aligned buffers")
        o_in = {k: v for k, v in (out or {}).items() if k != "B_hist"}
        r = run(variant, params, W_arg, S_arg, B_init, Wprev_init, want_hist=True, want=want, chunk_epochs=chunk_epochs,
                workspace=workspace, out=o_in or None, phase_ms=phase_ms, shared_inputs=shared_inputs, sched=sched)
        dense = r.B_hist
        if want_move:
            r.B_move = move_from_history(dense, None if B_init is None else _as_dev(B_init, dev))
            r.extra["move_path"] = "dense"
        if want_row_stats:
            r.B_rowstat = rowstat_from_history(dense, None if B_init is None else _as_dev(B_init, dev))
            r.extra["rowstat_path"] = "dense"
        slots = torch.as_tensor(h_epochs, dtype=torch.int64, device=dev)
        hist_user = (out or {}).get("B_hist")
        r.B_hist, r.hist_epochs = None, None
        if want_hist or hist_user is not None:
            h = dense if len(h_epochs) == E else dense.index_select(0, slots)
            if h_bf16:
                h = h.to(torch.bfloat16)
            if hist_user is not None:
                if hist_user.dtype != h.dtype or tuple(hist_user.shape) != tuple(h.shape):
                    raise ValueError(f"out['B_hist'] is {hist_user.dtype} {tuple(hist_user.shape)}, the history asked "
                                     f"for {h.dtype} {tuple(h.shape)}")
                h = hist_user.copy_(h)
            r.B_hist, r.hist_epochs = h, h_epochs
        if watch_host is not None:
            r.B_watch = dense.index_select(0, slots).index_select(3, watch_host.to(dev)).contiguous()
            r.watch_cols = tuple(int(c) for c in watch_host.tolist())
            r.hist_epochs = h_epochs
            r.extra["watch_path"], r.extra["watch"] = "dense", None
        if rows_host is not None:
            r.B_rows = dense.index_select(0, slots).index_select(2, rows_host.to(dev)).contiguous()
            r.watch_rows = tuple(int(c) for c in rows_host.tolist())
            r.hist_epochs = h_epochs
            r.extra["rows_path"], r.extra["watch_rows"] = "dense", None
        return r

    def segments():
        """the chain of existing runs that defines the events (nothing is launched yet)"""
        if capture is not None:
            raise EngineError("a captured run cannot cut itself at the event epochs: resets= needs "
                              "resets_native(variant, N, E, V, M, ...) and vector-aligned buffers")
        if phase_ms is not None:
            raise ValueError("phase_ms times one launch: the events of this call are not native")
        if resets is None:
            ev = torch.zeros((0, 4), dtype=torch.int64)
        else:
            ev = resets_host if resets_host is not None else resets.detach().to(device="cpu", dtype=torch.int64)
        row_ev = None
        if row_resets is not None:
            row_ev = rowev_host if rowev_host is not None else row_resets.detach().to(device="cpu", dtype=torch.int64)
            if row_ev.shape[1] == 3:
                row_ev = torch.cat([row_ev, torch.zeros((row_ev.shape[0], 1), dtype=torch.int64)], dim=1)
        return _run_segments(variant, params, W_arg, S_arg, B_init, Wprev_init, ev, N=N, E=E, M=M, h_epochs=h_epochs,
                             want_hist=want_hist or (out or {}).get("B_hist") is not None, want=want,
                             chunk_epochs=chunk_epochs, workspace=workspace, out=out, shared_inputs=shared_inputs,
                             hist_stride=hist_stride, row_ev=row_ev)

    out_names = tuple(want) + tuple(k for k, v in (out or {}).items() if v is not None and k != "B_hist")
    if resets is not None and not resets_native(variant, N, E, V, M, False, out_names, shared_inputs=shared_inputs,
                                                w_u16=W.dtype == torch.uint16):
        return segments()
    if row_resets is not None and not events_native(variant, N, E, V, M, False, out_names, shared_inputs=shared_inputs,
                                                    w_u16=W.dtype == torch.uint16):
        return segments()
    if want_move and (want_hist or (out or {}).get("B_hist") is not None
                      or not move_native(variant, N, E, V, M, False, out_names, shared_inputs=shared_inputs)):
        return move_dense()
    # the row summary: native alone; beside a history, a schedule, B_move or uint16 weights it is reduced
    if want_row_stats and (want_hist or (out or {}).get("B_hist") is not None or want_move or sched is not None
                           or W.dtype == torch.uint16
                           or not rowstat_native(variant, N, E, V, M, False, out_names, shared_inputs=shared_inputs)):
        return move_dense()
    # a watch list the engine does not take natively rides on an fp32 history of the run's own
    watch_dense = watch_host is not None and (
        single_call or not watch_native(variant, N, E, V, M, watch_host.numel(), shared_inputs=shared_inputs))
    if watch_dense and capture is not None:
        raise EngineError("a captured run cannot gather a dense history: watch= needs "
                          "watch_native(variant, N, E, V, M, n_watch)")
    # ... and so does a row list
    rows_dense = rows_host is not None and (
        single_call or not rows_native(variant, N, E, V, M, rows_host.numel(), shared_inputs=shared_inputs))
    if rows_dense and capture is not None:
        raise EngineError("a captured run cannot gather a dense history: watch_rows= needs "
                          "rows_native(variant, N, E, V, M, n_rows)")
    hist_asked = want_hist or (out or {}).get("B_hist") is not None
    if (watch_dense or rows_dense) and not hist_asked:
        want_hist, hist_dtype, h_bf16 = True, None, False  # (dropped again below)
    # uint16 weights stay 16-bit on the device where the engine reads them
    # natively (u16_native); anywhere else they are widened like any dtype
    w_u16 = False
    if W.dtype == torch.uint16:
        W = W.to(device=dev).contiguous()
        names = tuple(want) + tuple(k for k, v in (out or {}).items() if v is not None)
        w_u16 = (not single_call and W.data_ptr() % 8 == 0
                 and u16_native(variant, N, E, V, M, want_hist, names, shared_inputs=shared_inputs))
    if not w_u16:
        W = _as_dev(W, dev)
    S = _as_dev(S, dev)
    B_init = None if B_init is None else _as_dev(B_init, dev)
    Wprev_init = None if Wprev_init is None else _as_dev(Wprev_init, dev)
    prm = params_tensor(params, dev)
    o = {} if out is None else dict(out)
    sizes = {"E": E, "N": N, "V": V, "M": M, "2": 2}

    def need(name):
        if o.get(name) is None:
            o[name] = torch.empty(tuple(sizes[d] for d in _OUT_SHAPES[name]), dtype=torch.float32, device=dev)

    for name in ("Dn", "C", "I", "B_final"):
        need(name)
    hist_user = o.get("B_hist") if h_bf16 else None  # the caller's bfloat16 buffer: the result goes there
    hist_native = _alloc_history(
        o, dev, (len(h_epochs), N, V, M), want_hist=want_hist, h_bf16=h_bf16,
        native_ok=lambda: hist_bf16_native(variant, N, E, V, M, shared_inputs=shared_inputs))
    for name in want:
        need(name)
    if "T" in o and "P" not in o:
        need("P")
    # the three native paths need the vector form; each falls back where a buffer is off its alignment
    hist_native = hist_native and _vector_form(W, w_u16, B_init, Wprev_init, o, True)
    if h_bf16 and o.get("B_hist") is not None and not hist_native:
        if capture is not None:
            raise EngineError("a captured run cannot convert an fp32 history: hist_dtype=torch.bfloat16 needs "
                              "hist_bf16_native(variant, N, E, V, M), a stored epoch and vector-aligned buffers")
        if o["B_hist"].dtype != torch.float32:  # the run's fp32 history, converted below
            o["B_hist"] = torch.empty((len(h_epochs), N, V, M), dtype=torch.float32, device=dev)
    if w_u16 and not _vector_form(W, True, B_init, Wprev_init, o, hist_native):
        w_u16 = False
        W = _as_dev(W, dev)
    sched_dev = None
    if sched is not None:
        names = tuple(k for k, v in o.items() if v is not None and k != "B_hist")
        if (not single_call
                and sched_native(variant, N, E, K, V, M, o.get("B_hist") is not None, names,
                                 shared_inputs=shared_inputs)
                and _vector_form(W, w_u16, B_init, Wprev_init, o, hist_native)):
            if (isinstance(sched, torch.Tensor) and sched.device == dev and sched.dtype == torch.int32
                    and sched.is_contiguous()):
                sched_dev = sched  # the caller's tensor: a captured run follows its in-place updates
            else:
                sched_dev = sched_host.to(device=dev, dtype=torch.int32)
        else:
            if capture is not None:
                raise EngineError("a captured run cannot expand its inputs: sched= needs "
                                  "sched_native(variant, N, E, K, V, M, ...) and vector-aligned buffers")
            W, S = _take_slices(W, sched_host.to(dev)), _take_slices(S, sched_host.to(dev))
    if (want_move or want_row_stats) and not _vector_form(W, w_u16, B_init, Wprev_init, o, False):
        return move_dense()  # (nothing is launched yet)
    resets_dev = None
    rowev_dev = None
    if row_resets is not None:
        if not _vector_form(W, False, B_init, Wprev_init, o, False):  # (nothing is launched yet)
            return segments()
        if rowev_host is not None:
            rowev_dev = rowev_host.to(device=dev, dtype=torch.int32)
        elif row_resets.shape[1] == 3:  # 16-byte records: the reserved word added on the device
            rowev_dev = torch.nn.functional.pad(row_resets, (0, 1)).contiguous()
        else:
            rowev_dev = row_resets if row_resets.is_contiguous() else row_resets.contiguous()  # unchecked
    if resets is not None:
        if not _vector_form(W, False, B_init, Wprev_init, o, False):  # (nothing is launched yet)
            return segments()
        if resets_host is None:
            resets_dev = resets if resets.is_contiguous() else resets.contiguous()  # the caller's tensor, unchecked
        else:
            resets_dev = resets_host.to(device=dev, dtype=torch.int32)
    b_move = torch.empty((E, N, 2), dtype=torch.float32, device=dev) if want_move else None  # (the engine zeroes it)
    b_rowstat = torch.empty((E, N, V, 3), dtype=torch.float32, device=dev) if want_row_stats else None  # (likewise)
    watch_arg = None
    if watch_host is not None and not watch_dense:
        if (isinstance(watch, torch.Tensor) and watch.device == dev and watch.dtype == torch.int32
                and watch.is_contiguous()):
            watch_dev = watch  # the caller's tensor: a captured run follows its in-place updates
        else:
            watch_dev = watch_host.to(device=dev, dtype=torch.int32)
        b_watch = torch.empty((len(h_epochs), N, V, watch_host.numel()), dtype=torch.float32, device=dev)
        # (no stored epoch: nothing is written, but the engine refuses a null B_watch)
        watch_arg = (watch_dev, b_watch, b_watch if h_epochs else torch.empty(1, dtype=torch.float32, device=dev))
    rows_arg = None
    if rows_host is not None and not rows_dense:
        if (isinstance(watch_rows, torch.Tensor) and watch_rows.device == dev and watch_rows.dtype == torch.int32
                and watch_rows.is_contiguous()):
            rows_dev = watch_rows  # the caller's tensor: a captured run follows its in-place updates
        else:
            rows_dev = rows_host.to(device=dev, dtype=torch.int32)
        b_rows = torch.empty((len(h_epochs), N, rows_host.numel(), M), dtype=torch.float32, device=dev)
        # (no stored epoch: nothing is written, but the engine refuses a null B_rows)
        rows_arg = (rows_dev, b_rows, b_rows if h_epochs else torch.empty(4, dtype=torch.float32, device=dev))
    outs = YumaOutputsC(**{k: _ptr(o.get(k)) for k in OUTPUT_FIELDS})
    # the run as one record: the sizes and sections size the workspace, then the record is the launch
    req = YumaRequestC(struct_size=ctypes.sizeof(YumaRequestC), variant=variant, N=N, E=E, V=V, M=M,
                       params_dev=prm.data_ptr(), W=W.data_ptr(), S=S.data_ptr(), B_init=_ptr(B_init),
                       Wprev_init=_ptr(Wprev_init), out=ctypes.addressof(outs), chunk_epochs=int(chunk_epochs))
    if sched_dev is not None:
        req.K, req.sched_dev = K, sched_dev.data_ptr()
    _list_section(req, REQ_WATCH, ("watch_dev", "n_watch", "B_watch"), watch_arg)
    _list_section(req, REQ_ROWS, ("rows_dev", "n_rows", "B_rows"), rows_arg)
    if b_move is not None:
        req.sections, req.B_move = req.sections | REQ_MOVE, b_move.data_ptr()
    if b_rowstat is not None:
        req.sections, req.B_rowstat = req.sections | REQ_ROWSTAT, b_rowstat.data_ptr()
    _events_section(req, REQ_RESETS, ("events_dev", "n_events"), resets_dev)
    _events_section(req, REQ_ROW_EVENTS, ("row_events_dev", "n_row_events"), rowev_dev)
    if not hasattr(lib, "yuma_run_request"):
        raise EngineUnavailable("this library has no yuma_run_request: it was built from older sources; run it with "
                                "the engine.py of those sources")
    nbytes = int(lib.yuma_workspace_bytes_request(ctypes.addressof(req)))
    if workspace is None or workspace.numel() < nbytes:
        workspace = torch.empty(max(nbytes, 1), dtype=torch.uint8, device=dev)
    req.workspace, req.workspace_bytes = workspace.data_ptr(), workspace.numel()
    if single_call:  # one Yuma* call per slice: the yuma_epoch entry point
        if E != 1 or capture is not None or phase_ms is not None:
            raise ValueError("single_call is one epoch, launched directly")
        _check(lib.yuma_epoch(variant, prm.data_ptr(), N, V, M, W.data_ptr(), _ptr(Wprev_init),
                              S.data_ptr(), _ptr(B_init), ctypes.addressof(outs), workspace.data_ptr(),
                              workspace.numel(), torch.cuda.current_stream(dev).cuda_stream), "yuma_epoch")
    else:
        opts = YumaRunOptionsC(flags=(RUN_SHARED_INPUTS if shared_inputs else 0) | (RUN_W_U16 if w_u16 else 0)
                               | (RUN_HIST_BF16 if hist_native else 0),
                               # (a stride of E or more stores one epoch at the most: int32 either way)
                               hist_stride=min(int(hist_stride), E), hist_first=h_epochs[0] if h_epochs else E)
        req.opts = ctypes.addressof(opts)
        _launch(lib, dev, req, capture=capture, phase_ms=phase_ms)
    keep = {k: v for k, v in o.items() if k not in ("Dn", "C", "I", "B_final", "B_hist")}
    # keep inputs alive until the stream has consumed them
    keep["_inputs"] = (W, S, B_init, Wprev_init, prm, workspace)
    keep["w_path"] = "u16" if w_u16 else "f32"  # how W was read: natively as uint16, or as fp32
    keep["hist_path"] = "bf16" if hist_native else "f32"  # how the scan wrote the history
    if sched is not None:  # how the schedule was taken: by the engine, or expanded to a slice per epoch
        keep["sched_path"] = "native" if sched_dev is not None else "expanded"
        keep["sched"] = sched_dev
    if want_move:
        keep["move_path"] = "native"
    if want_row_stats:
        keep["rowstat_path"] = "native"
    if resets is not None:  # how the events were applied: by the bond scan, or by cutting the run
        keep["resets_path"] = "native"
        keep["resets"] = resets_dev
    if row_resets is not None:
        keep["resets_path"] = "native"
        keep["row_resets"] = rowev_dev
    hist = o.get("B_hist")
    if h_bf16 and hist is not None and not hist_native:  # the fp32 history, rounded to nearest even
        hist = hist.to(torch.bfloat16) if hist_user is None else hist_user.copy_(hist)
    if watch_host is None and rows_host is None:
        return RunResult(o["Dn"], o["C"], o["I"], o["B_final"], hist, keep, None if hist is None else h_epochs,
                         B_move=b_move, B_rowstat=b_rowstat)
    if (watch_dense or rows_dense) and not hist_asked:  # the history was the run's own: dropped
        hist = None
    if watch_host is None:
        b_watch = None
    else:
        keep["watch_path"] = "dense" if watch_dense else "native"
        keep["watch"] = None if watch_dense else watch_dev
        if watch_dense:  # the columns of the run's fp32 history (o: before any bfloat16 conversion)
            b_watch = o["B_hist"].index_select(3, watch_host.to(dev)).contiguous()
    if rows_host is None:
        b_rows = None
    else:
        keep["rows_path"] = "dense" if rows_dense else "native"
        keep["watch_rows"] = None if rows_dense else rows_dev
        if rows_dense:  # the rows of the run's fp32 history
            b_rows = o["B_hist"].index_select(2, rows_host.to(dev)).contiguous()
    return RunResult(o["Dn"], o["C"], o["I"], o["B_final"], hist, keep, h_epochs, b_watch,
                     None if watch_host is None else tuple(int(c) for c in watch_host.tolist()), B_move=b_move,
                     B_rows=b_rows, watch_rows=None if rows_host is None else tuple(int(c) for c in rows_host.tolist()),
                     B_rowstat=b_rowstat)


class RunGraph:
    """A whole `run` captured once into a HIP graph (yuma_graph_create_request) and
    replayed with one launch per call: the E-epoch loop of run_simulation
    (simulation_utils.py:52-110) with no host work between phases or epochs.
    Inputs and outputs are the buffers of the capture (`result`); refill the
    inputs in place between replays."""

    def __init__(self, variant: int, params: list[YumaParamsC], W: torch.Tensor, S: torch.Tensor,
                 B_init: torch.Tensor | None = None, Wprev_init: torch.Tensor | None = None, **kw):
        self._lib = load_library()
        h: list = []
        self.result = run(variant, params, W, S, B_init, Wprev_init, capture=h, **kw)
        self._h = h[0]

    def launch(self) -> RunResult:
        stream = torch.cuda.current_stream(device()).cuda_stream
        _check(self._lib.yuma_graph_launch(self._h, stream), "yuma_graph_launch")
        return self.result

    def nodes(self) -> int:
        return int(self._lib.yuma_graph_nodes(self._h))

    def close(self) -> None:
        if self._h is not None:
            self._lib.yuma_graph_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


def shard_stage(stage: int, variant: int, prm: torch.Tensor, W: torch.Tensor, S: torch.Tensor,
                B_init: torch.Tensor | None, Wprev_init: torch.Tensor | None, *, M_total: int,
                col0: int, io: dict, out: dict, workspace: torch.Tensor) -> None:
    """One stage of a miner-column-sharded run (yuma_shard_stage). W [E,N,V,M]
    holds this shard's columns; `io` maps SHARD_IO_FIELDS to device tensors;
    `out` maps OUTPUT_FIELDS to device tensors (local columns)."""
    lib = load_library()
    E, N, V, M = W.shape
    for k in io:
        if k not in SHARD_IO_FIELDS:
            raise KeyError(f"unknown shard io field {k}")
    cio = YumaShardIOC(M_total=int(M_total), col0=int(col0),
                       **{k: _ptr(io.get(k)) for k in SHARD_IO_FIELDS})
    outs = YumaOutputsC(**{k: _ptr(out.get(k)) for k in OUTPUT_FIELDS})
    stream = torch.cuda.current_stream(W.device).cuda_stream
    _check(lib.yuma_shard_stage(stage, variant, prm.data_ptr(), N, E, V, M, W.data_ptr(),
                                S.data_ptr(), _ptr(B_init), _ptr(Wprev_init),
                                ctypes.addressof(cio), ctypes.addressof(outs),
                                workspace.data_ptr(), workspace.numel(), stream),
           f"yuma_shard_stage({stage})")


def synth_weights(seed: int, E: int, N: int, V: int, M: int, t0: int = 0,
                  out: torch.Tensor | None = None) -> torch.Tensor:
    """Device twin of synth.weights (bit-identical)."""
    dev = device()
    if out is None:
        out = torch.empty((E, N, V, M), dtype=torch.float32, device=dev)
    stream = torch.cuda.current_stream(dev).cuda_stream
    _check(load_library().yuma_synth_weights(int(seed) & 0xFFFFFFFFFFFFFFFF, E, N, V, M, t0,
                                             out.data_ptr(), stream), "yuma_synth_weights")
    return out


def version() -> str:
    return load_library().yuma_version().decode()


def build_id() -> str:
    """The library's source identity (yuma_build_id: "src-" + SHA-256 prefix of
    the engine source and header it was built from)."""
    lib = load_library()
    return lib.yuma_build_id().decode() if hasattr(lib, "yuma_build_id") else "unstamped"

