"""What a bfloat16 bond history costs or saves at the c2 shape, one process,
one build.

The synthetic inputs are bench.py's c2 (same seed). Per version -- Yuma 3 and
Yuma 4 liquid alpha -- four graphs are built over the same inputs: the fp32
dense history, the bfloat16 dense history, the bfloat16 history at stride 10,
and no history. After a clock ramp and warm-up they are replayed in turn
(A, B, C, D, A, ...) with a device-event time per replay: each mode's median
and min-max in ms per step, then the bond phase's HIP-event time of a direct
run of each (phase_ms). Before anything is timed every bfloat16 history is
compared bit for bit with the fp32 one rounded to nearest even at its stored
epochs, and the other outputs with the fp32-history run's. Prints one JSON
line.

    python tools/bench_hist_bf16.py [--replays 24] [--warmup 5] [--stride 10]
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
BF16 = torch.bfloat16


def spread(xs):
    return {"median_ms": round(statistics.median(xs), 4), "min_ms": round(min(xs), 4), "max_ms": round(max(xs), 4),
            "n": len(xs)}


def main():
    ap = argparse.ArgumentParser(description=__doc__.splitlines()[0])
    ap.add_argument("--replays", type=int, default=24, help="timed replays per mode (>= 4)")
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--phase-reps", type=int, default=3)
    ap.add_argument("--stride", type=int, default=10)
    a = ap.parse_args()
    dev = engine.device()
    W = engine.synth_weights(SEED, E, N, V, M)
    S = torch.from_numpy(synth.stakes(SEED, E, N, V)).to(dev)
    ws = torch.empty(engine.workspace_bytes(engine.VARIANT_YUMA4, N, E, V, M, False), dtype=torch.uint8, device=dev)
    # mode -> engine.run keywords
    modes = {"f32_dense": dict(want_hist=True),
             "bf16_dense": dict(want_hist=True, hist_dtype=BF16),
             f"bf16_stride_{a.stride}": dict(want_hist=True, hist_dtype=BF16, hist_stride=a.stride),
             "no_history": dict(want_hist=False)}

    def hist_bytes(kw):
        if not kw["want_hist"]:
            return 0
        return len(engine.hist_epochs(E, kw.get("hist_stride", 1))) * N * V * M * (2 if "hist_dtype" in kw else 4)

    line = {"tool": "bench_hist_bf16", "shape": {"V": V, "M": M, "epochs": E, "scenarios": N},
            "engine_build_id": engine.build_id(), "launch": "hipGraph replay, modes in turn",
            "hist_bytes": {m: hist_bytes(kw) for m, kw in modes.items()}, "versions": {}}
    for name, variant, liquid in VERSIONS:
        params = [engine.make_params(variant, YumaConfig(yuma_params=YumaParams(liquid_alpha=liquid)))]
        graphs = {m: engine.RunGraph(variant, params, W, S, workspace=ws, **kw) for m, kw in modes.items()}
        res = {m: g.launch() for m, g in graphs.items()}
        torch.cuda.synchronize()
        ref = res["f32_dense"]
        for m, r in res.items():
            ok = all(torch.equal(getattr(r, k), getattr(ref, k)) for k in ("Dn", "C", "I", "B_final"))
            if r.B_hist is not None and r.B_hist.dtype == BF16:
                ok = ok and r.extra["hist_path"] == "bf16"
                ok = ok and all(torch.equal(r.B_hist[j].view(torch.int16), ref.B_hist[t].to(BF16).view(torch.int16))
                                for j, t in enumerate(r.hist_epochs))
            if not ok:
                raise SystemExit(f"{name}: {m} differs from the fp32-history run")
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
        for _ in range(max(a.replays, 4)):
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
        line["versions"][name] = {"step": {m: spread(t) for m, t in times.items()}, "bonds_phase_ms": bonds,
                                  "outputs_bit_equal": True}
        for g in graphs.values():
            g.close()
        del graphs, res, ref
        torch.cuda.empty_cache()
    print(json.dumps(line), flush=True)


if __name__ == "__main__":
    main()
