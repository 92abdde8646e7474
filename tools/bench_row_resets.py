"""What validator-row events cost at the c2 shape, one process, one build.

The synthetic inputs are bench.py's c2 (same seed), with a dense fp32 bond
history. Per version -- Yuma 3 and Yuma 4 liquid alpha -- four graphs are built
over the same inputs: the plain run; the RL run with an empty-but-present
column table (resets= with one out-of-range event: the scan the row form is
judged against); the RW run with both tables empty (row_resets= with one
out-of-range event: what the second table costs); one row event per epoch.
After a clock ramp and warm-up they are replayed in turn (A, B, C, D, A, ...)
with a device-event time per replay: each mode's median and min-max in ms per
step. The two empty-table runs are compared bit for bit with the plain run
before anything is timed. Then, on the first tenth of the epochs and the
one-event-per-epoch list, the native direct run is timed against the
"segments" chain (the cut-and-resume runs the events replace), both wall-clock
with a device synchronisation, after comparing their outputs bit for bit.
Exits non-zero unless the native run is shorter than the chain with
non-overlapping ranges, for both versions. Prints one JSON line.

    python tools/bench_row_resets.py [--replays 24] [--warmup 5] [--chain-reps 3]
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
ALWAYS = engine.RESET_ALWAYS


def spread(xs):
    return {"median_ms": round(statistics.median(xs), 4), "min_ms": round(min(xs), 4), "max_ms": round(max(xs), 4),
            "n": len(xs)}


def events(per_epoch, epochs=E):
    """per_epoch row events at every epoch from 1, validators spread over the rows"""
    return [(t, 0, (t * 131 + k * 61) % V, 0) for t in range(1, epochs) for k in range(per_epoch)]


def main():
    ap = argparse.ArgumentParser(description=__doc__.splitlines()[0])
    ap.add_argument("--replays", type=int, default=24, help="timed replays per mode (>= 24)")
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--chain-reps", type=int, default=3)
    a = ap.parse_args()
    dev = engine.device()
    W = engine.synth_weights(SEED, E, N, V, M)
    S = torch.from_numpy(synth.stakes(SEED, E, N, V)).to(dev)
    lists = {"plain": None, "rl_empty": ("resets", [(E, 0, 0, ALWAYS)]), "rw_empty": ("row_resets", [(E, 0, 0, 0)]),
             "rw_1_per_epoch": ("row_resets", events(1))}
    lists = {m: None if ev is None else (ev[0], torch.tensor(ev[1], dtype=torch.int32, device=dev))
             for m, ev in lists.items()}
    line = {"tool": "bench_row_resets", "shape": {"V": V, "M": M, "epochs": E, "scenarios": N, "bond_history": True},
            "engine_build_id": engine.build_id(), "launch": "hipGraph replay, modes in turn",
            "scan": engine.scan_plan(engine.VARIANT_YUMA3, N, E, V, M, True).shape, "versions": {}}
    E10 = E // 10
    for name, variant, liquid in VERSIONS:
        params = [engine.make_params(variant, YumaConfig(yuma_params=YumaParams(liquid_alpha=liquid)))]
        graphs = {m: engine.RunGraph(variant, params, W, S, want_hist=True, **({} if ev is None else {ev[0]: ev[1]}))
                  for m, ev in lists.items()}
        res = {m: g.launch() for m, g in graphs.items()}
        torch.cuda.synchronize()
        for k in ("Dn", "C", "I", "B_final", "B_hist"):
            for m in ("rl_empty", "rw_empty"):
                if not torch.equal(getattr(res[m], k), getattr(res["plain"], k)):
                    raise SystemExit(f"{name}: the empty-table run {m} differs from the plain run in {k}")
        if any(r.extra.get("resets_path", "native") != "native" for r in res.values()):
            raise SystemExit(f"{name}: a run with events did not take the native path")
        changed = not torch.equal(res["rw_1_per_epoch"].B_final, res["plain"].B_final)
        t_end = time.perf_counter() + 1.0  # clock ramp (bench.py PREWARM_S)
        while time.perf_counter() < t_end:
            for g in graphs.values():
                g.launch()
            torch.cuda.synchronize()
        for _ in range(a.warmup):
            for g in graphs.values():
                g.launch()
        torch.cuda.synchronize()
        times = {m: [] for m in lists}
        ev = [torch.cuda.Event(enable_timing=True) for _ in range(len(lists) + 1)]
        for _ in range(max(a.replays, 24)):
            ev[0].record()
            for i, g in enumerate(graphs.values()):
                g.launch()
                ev[i + 1].record()
            torch.cuda.synchronize()
            for i, m in enumerate(lists):
                times[m].append(ev[i].elapsed_time(ev[i + 1]))
        for g in graphs.values():
            g.close()
        del graphs, res
        torch.cuda.empty_cache()
        # the chain the events replace, on a tenth of the epochs: one-epoch runs, wall-clock
        W10, S10, ev10 = W[:E10], S[:E10], events(1, E10)
        dev10 = torch.tensor(ev10, dtype=torch.int32, device=dev)
        host10 = torch.tensor(ev10, dtype=torch.int64)
        none10 = torch.zeros((0, 4), dtype=torch.int64)
        h10 = engine.hist_epochs(E10)

        def native():
            return engine.run(variant, params, W10, S10, row_resets=dev10, want_hist=True)

        def segments():
            return engine._run_segments(variant, params, W10, S10, None, None, none10, N=N, E=E10, M=M, h_epochs=h10,
                                        want_hist=True, want=(), chunk_epochs=0, workspace=None, out=None,
                                        shared_inputs=False, hist_stride=1, row_ev=host10)

        rn, rs = native(), segments()
        torch.cuda.synchronize()
        if rn.extra["resets_path"] != "native" or rs.extra["resets_path"] != "segments":
            raise SystemExit(f"{name}: unexpected paths")
        for k in ("Dn", "C", "I", "B_final", "B_hist"):
            if not torch.equal(getattr(rn, k), getattr(rs, k)):
                raise SystemExit(f"{name}: the native run differs from the segments chain in {k}")
        del rn, rs
        wall = {"native": [], "segments": []}
        for _ in range(max(a.chain_reps, 3)):
            for m, f in (("native", native), ("segments", segments)):
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                r = f()
                torch.cuda.synchronize()
                wall[m].append((time.perf_counter() - t0) * 1e3)
                del r
        step = {m: spread(t) for m, t in times.items()}
        tenth = {m: spread(t) for m, t in wall.items()}
        line["versions"][name] = {
            "step": step, "events_changed_B_final": changed, "outputs_bit_equal": True,
            "rl_minus_plain_ms": round(step["rl_empty"]["median_ms"] - step["plain"]["median_ms"], 4),
            "rw_minus_rl_ms": round(step["rw_empty"]["median_ms"] - step["rl_empty"]["median_ms"], 4),
            "one_per_epoch_minus_rw_empty_ms": round(step["rw_1_per_epoch"]["median_ms"] - step["rw_empty"]["median_ms"], 4),
            "tenth_of_the_epochs_wall": tenth,
            "native_below_segments": tenth["native"]["max_ms"] < tenth["segments"]["min_ms"]}
        torch.cuda.empty_cache()
    print(json.dumps(line), flush=True)
    if not all(v["native_below_segments"] for v in line["versions"].values()):
        raise SystemExit("the native run with events is not below the segments chain with non-overlapping ranges")


if __name__ == "__main__":
    main()
