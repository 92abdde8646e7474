"""What an input schedule costs and buys at the c2 shape, one process, one build.

The synthetic inputs are bench.py's c2 (same seed). Per version -- Yuma 3 with
the bond history and Yuma 4 liquid alpha with it -- five graphs are built:
  dense     K = E through today's entry point (one slice per epoch)
  identity  K = E through the schedule entry point, sched = 0 .. E-1: the cost
            of the mechanism itself (staging, the gather, the scalar index load)
  k100, k10, k1   the first K slices held for E / K epochs each (block schedules)
Every schedule run is first compared bit for bit, every output, with a dense run
on its expanded inputs. After a clock ramp and warm-up the graphs are replayed
in turn (A, B, C, D, E, A, ...) with a device-event time per replay: each
mode's median and min-max in ms per replay, then the per-phase HIP-event times
of a direct run of each (phase_ms; the gather is counted under "incentive").
Prints one JSON line.

    python tools/bench_sched.py [--replays 24] [--warmup 5] [--ks 100,10,1]
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
FIELDS = ("Dn", "C", "I", "B_final", "B_hist")


def spread(xs):
    return {"median_ms": round(statistics.median(xs), 4), "min_ms": round(min(xs), 4), "max_ms": round(max(xs), 4),
            "n": len(xs)}


def main():
    ap = argparse.ArgumentParser(description=__doc__.splitlines()[0])
    ap.add_argument("--replays", type=int, default=24, help="timed replays per mode (>= 20)")
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--phase-reps", type=int, default=3)
    ap.add_argument("--ks", default="100,10,1")
    a = ap.parse_args()
    ks = [int(k) for k in a.ks.split(",")]
    dev = engine.device()
    W = engine.synth_weights(SEED, E, N, V, M)
    S = torch.from_numpy(synth.stakes(SEED, E, N, V)).to(dev)
    # mode -> (stored slices, schedule or None)
    modes = {"dense": (E, None), "identity": (E, torch.arange(E, dtype=torch.int32, device=dev))}
    for k in ks:
        modes[f"k{k}"] = (k, (torch.arange(E, device=dev) * k // E).to(torch.int32))

    line = {"tool": "bench_sched", "shape": {"V": V, "M": M, "epochs": E, "scenarios": N},
            "engine_build_id": engine.build_id(), "launch": "hipGraph replay, modes in turn",
            "w_bytes": {m: k * N * V * M * 4 for m, (k, _) in modes.items()},
            "workspace_bytes": {m: (engine.workspace_bytes(engine.VARIANT_YUMA4, N, E, V, M, False) if s is None else
                                    engine.workspace_bytes_sched(engine.VARIANT_YUMA4, N, E, k, V, M, False))
                                for m, (k, s) in modes.items()},
            "versions": {}}
    for name, variant, liquid in VERSIONS:
        params = [engine.make_params(variant, YumaConfig(yuma_params=YumaParams(liquid_alpha=liquid)))]
        kw = {m: dict(want_hist=True) if s is None else dict(want_hist=True, sched=s) for m, (k, s) in modes.items()}
        graphs = {m: engine.RunGraph(variant, params, W[:k], S[:k], **kw[m]) for m, (k, _) in modes.items()}
        res = {m: g.launch() for m, g in graphs.items()}
        torch.cuda.synchronize()
        for m, (k, s) in modes.items():
            if s is None:
                continue
            if res[m].extra["sched_path"] != "native":
                raise SystemExit(f"{name}: {m} did not take the schedule natively")
            ref = res["dense"] if m == "identity" else engine.run(
                variant, params, W[:k].index_select(0, s.long()), S[:k].index_select(0, s.long()), want_hist=True)
            torch.cuda.synchronize()
            if not all(torch.equal(getattr(res[m], f), getattr(ref, f)) for f in FIELDS):
                raise SystemExit(f"{name}: {m} differs from the dense run on its expanded inputs")
            del ref
            torch.cuda.empty_cache()
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
        for _ in range(max(a.replays, 20)):
            ev[0].record()
            for i, g in enumerate(graphs.values()):
                g.launch()
                ev[i + 1].record()
            torch.cuda.synchronize()
            for i, m in enumerate(modes):
                times[m].append(ev[i].elapsed_time(ev[i + 1]))
        phases = {}
        for m, (k, _) in modes.items():
            po = {f: getattr(res[m], f) for f in FIELDS}
            reps = []
            for _ in range(a.phase_reps + 1):
                buf: list = []
                engine.run(variant, params, W[:k], S[:k], out=po, phase_ms=buf, **kw[m])
                reps.append(buf)
            # the first direct run warms the non-graph launch path
            phases[m] = {p: round(statistics.median(r[i] for r in reps[1:]), 4) for i, p in enumerate(engine.PHASES)}
        line["versions"][name] = {"replay": {m: spread(t) for m, t in times.items()}, "phase_ms": phases,
                                  "outputs_bit_equal": True}
        for g in graphs.values():
            g.close()
        del graphs, res
        torch.cuda.empty_cache()
    print(json.dumps(line), flush=True)


if __name__ == "__main__":
    main()
