"""What the per-validator bond summary costs at the c2 shape, one process, one build.

The synthetic inputs are bench.py's c2 (same seed). Per version -- Yuma 3 and
Yuma 4 liquid alpha -- four graphs are built over the same inputs: no history,
no history with want_move, no history with want_row_stats (the history-less
scan forms B_rowstat [E, N, V, 3] itself), and the dense fp32 bond history
(what B_rowstat replaces). After a clock ramp and warm-up they are replayed in
turn (A, B, C, D, A, ...) with a device-event time per replay: each mode's
median and min-max in ms per step, then the bond phase's HIP-event time of a
direct run of each (phase_ms). Columns 0 and 1 of B_rowstat are compared bit
for bit with the definition on the dense history, their maximum over the
validators with B_move, column 2 with the float64 row sums under the (M - 1)
2^-24 bound, and every other output with the dense run's, before anything is
timed. Prints one JSON line, which says whether the want_row_stats step is
shorter than the dense-history step with non-overlapping ranges.

    python tools/bench_rowstat.py [--replays 24] [--warmup 5]
"""

from __future__ import annotations

import argparse
import json
import os
import statistics
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "yuma-simulation_amd")):
    if p not in sys.path:
        sys.path.insert(0, p)

from yuma_simulation._internal import engine, synth  # noqa: E402
from yuma_simulation._internal.yumas import YumaConfig, YumaParams  # noqa: E402

E, V, M, N = 1000, 256, 4096, 1  # bench.py DEFAULTS["c2"]
SEED = 0x5EED0002                # ... and its c2 seed
VERSIONS = [("Yuma 3 (Rhef)", engine.VARIANT_YUMA3, False),
            ("Yuma 4 (Rhef+relative bonds) - liquid alpha on", engine.VARIANT_YUMA4, True)]


def spread(xs):
    return {"median_ms": round(statistics.median(xs), 4), "min_ms": round(min(xs), 4), "max_ms": round(max(xs), 4),
            "n": len(xs)}


def main():
    ap = argparse.ArgumentParser(description=__doc__.splitlines()[0])
    ap.add_argument("--replays", type=int, default=24, help="timed replays per mode (>= 24)")
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--phase-reps", type=int, default=3)
    a = ap.parse_args()
    dev = engine.device()
    W = engine.synth_weights(SEED, E, N, V, M)
    S = torch.from_numpy(synth.stakes(SEED, E, N, V)).to(dev)
    ws = torch.empty(engine.workspace_bytes_rowstat(engine.VARIANT_YUMA4, N, E, V, M, False), dtype=torch.uint8, device=dev)
    # mode -> engine.run keywords
    modes = {"no_history": dict(want_hist=False), "move": dict(want_hist=False, want_move=True),
             "row_stats": dict(want_hist=False, want_row_stats=True), "dense": dict(want_hist=True)}
    line = {"tool": "bench_rowstat", "shape": {"V": V, "M": M, "epochs": E, "scenarios": N},
            "engine_build_id": engine.build_id(), "launch": "hipGraph replay, modes in turn",
            "scan": engine.scan_plan(engine.VARIANT_YUMA3, N, E, V, M).shape, "versions": {}}
    for name, variant, liquid in VERSIONS:
        params = [engine.make_params(variant, YumaConfig(yuma_params=YumaParams(liquid_alpha=liquid)))]
        graphs = {m: engine.RunGraph(variant, params, W, S, workspace=ws, **kw) for m, kw in modes.items()}
        res = {m: g.launch() for m, g in graphs.items()}
        torch.cuda.synchronize()
        dense = res["dense"]
        for m, r in res.items():
            if not all(torch.equal(getattr(r, k), getattr(dense, k)) for k in ("Dn", "C", "I", "B_final")):
                raise SystemExit(f"{name}: {m} differs from the dense run")
        mv, rs = res["move"], res["row_stats"]
        want = engine.rowstat_from_history(dense.B_hist, None)
        if rs.extra["rowstat_path"] != "native" or rs.B_hist is not None or not torch.equal(rs.B_rowstat[..., :2], want[..., :2]):
            raise SystemExit(f"{name}: B_rowstat's maxima differ from the dense history's")
        if not torch.equal(rs.B_rowstat[..., :2].amax(2), mv.B_move):
            raise SystemExit(f"{name}: the maximum of B_rowstat over the validators differs from B_move")
        ref = dense.B_hist.double().sum(-1)
        if not bool(((rs.B_rowstat[..., 2].double() - ref).abs() <= (M - 1) * 2.0 ** -24 * ref).all()):
            raise SystemExit(f"{name}: a row total is outside (M - 1) 2^-24 of the float64 sum")
        settled = engine.settled_epoch_rows(rs.B_rowstat, 1e-6, relative=True)[0]
        settled = {"first": int(settled.min()), "last": int(settled.max())}
        del want, ref
        t_end = time.perf_counter() + 1.0  # clock ramp (bench.py PREWARM_S)
        while time.perf_counter() < t_end:
            for g in graphs.values():
                g.launch()
            torch.cuda.synchronize()
        for _ in range(a.warmup):
            for g in graphs.values():
                g.launch()
        torch.cuda.synchronize()
        times = {m: [] for m in modes}
        ev = [torch.cuda.Event(enable_timing=True) for _ in range(len(modes) + 1)]
        for _ in range(max(a.replays, 24)):
            ev[0].record()
            for i, g in enumerate(graphs.values()):
                g.launch()
                ev[i + 1].record()
            torch.cuda.synchronize()
            for i, m in enumerate(modes):
                times[m].append(ev[i].elapsed_time(ev[i + 1]))
        bonds = {}
        bi = engine.PHASES.index("bonds")
        for m, kw in modes.items():
            po = {k: getattr(res[m], k) for k in ("Dn", "C", "I", "B_final", "B_hist") if getattr(res[m], k) is not None}
            reps = []
            for _ in range(a.phase_reps + 1):
                buf: list = []
                engine.run(variant, params, W, S, out=po, workspace=ws, phase_ms=buf, **kw)
                reps.append(buf[bi])
            bonds[m] = round(statistics.median(reps[1:]), 4)  # the first direct run warms the non-graph launch path
        step = {m: spread(t) for m, t in times.items()}
        line["versions"][name] = {
            "step": step, "bonds_phase_ms": bonds, "outputs_bit_equal": True,
            "row_stats_minus_no_history_ms": round(step["row_stats"]["median_ms"] - step["no_history"]["median_ms"], 4),
            "row_stats_minus_move_ms": round(step["row_stats"]["median_ms"] - step["move"]["median_ms"], 4),
            "settled_epoch_rows_rel_1e-6": settled,
            "row_stats_below_dense": step["row_stats"]["max_ms"] < step["dense"]["min_ms"]}
        for g in graphs.values():
            g.close()
        del graphs, res, dense, mv, rs
        torch.cuda.empty_cache()
    print(json.dumps(line), flush=True)


if __name__ == "__main__":
    main()
