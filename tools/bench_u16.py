"""uint16 against fp32 weights at the c2 shape, one process, one build.

The synthetic inputs are bench.py's c2 (same seed; the weights are integers
<= 4095, so the uint16 copy holds the same values). Per version -- Yuma 3 with
the bond history and Yuma 4 liquid alpha -- one fp32 graph and one uint16
graph are built and, after a clock ramp and warm-up, replayed alternately
A, B, A, B ... with a device-event time per replay: each side's median and
min-max, then per-phase HIP-event times of a direct run of each
(yuma_run_profiled / yuma_run_ex phase_ms). The outputs of the two graphs are
compared bit for bit before anything is timed. Prints one JSON line.

    python tools/bench_u16.py [--replays 24] [--warmup 5]
    python tools/bench_u16.py --profile u16|f32 [--version-index 0]
        a few replays of ONE graph and nothing else: the command a rocprofv3
        counter pass wraps (FETCH_SIZE and WRITE_SIZE in runs of their own)
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


def outputs(dev):
    return {"Dn": torch.empty(E, N, V, device=dev), "C": torch.empty(E, N, M, device=dev),
            "I": torch.empty(E, N, M, device=dev), "B_final": torch.empty(N, V, M, device=dev),
            "B_hist": torch.empty(E, N, V, M, device=dev)}


def spread(xs):
    return {"median_ms": round(statistics.median(xs), 4), "min_ms": round(min(xs), 4), "max_ms": round(max(xs), 4),
            "n": len(xs)}


def main():
    ap = argparse.ArgumentParser(description=__doc__.splitlines()[0])
    ap.add_argument("--replays", type=int, default=24, help="timed replays per side (>= 20)")
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--phase-reps", type=int, default=3)
    ap.add_argument("--profile", choices=("u16", "f32"), default=None)
    ap.add_argument("--version-index", type=int, default=0)
    a = ap.parse_args()
    dev = engine.device()
    W32 = engine.synth_weights(SEED, E, N, V, M)
    assert float(W32.max()) <= 65535.0 and float(W32.min()) >= 0.0
    # (values <= 4095: through int16, whose device conversions every torch build has)
    W16 = W32.to(torch.int16).view(torch.uint16)
    S = torch.from_numpy(synth.stakes(SEED, E, N, V)).to(dev)
    ws = torch.empty(engine.workspace_bytes(engine.VARIANT_YUMA4, N, E, V, M, False), dtype=torch.uint8, device=dev)

    def graph(variant, params, W):
        return engine.RunGraph(variant, params, W, S, want_hist=True, out=outputs(dev), workspace=ws)

    if a.profile is not None:
        name, variant, liquid = VERSIONS[a.version_index]
        params = [engine.make_params(variant, YumaConfig(yuma_params=YumaParams(liquid_alpha=liquid)))]
        g = graph(variant, params, W16 if a.profile == "u16" else W32)
        assert g.result.extra["w_path"] == a.profile
        for _ in range(6):
            g.launch()
        torch.cuda.synchronize()
        print(json.dumps({"profile": a.profile, "version": name, "engine_build_id": engine.build_id()}), flush=True)
        return

    line = {"tool": "bench_u16", "shape": {"V": V, "M": M, "epochs": E, "scenarios": N, "bond_history": True},
            "engine_build_id": engine.build_id(), "launch": "hipGraph replay, interleaved f32/u16",
            "w_bytes": {"f32": W32.numel() * 4, "u16": W16.numel() * 2}, "versions": {}}
    for name, variant, liquid in VERSIONS:
        params = [engine.make_params(variant, YumaConfig(yuma_params=YumaParams(liquid_alpha=liquid)))]
        ga, gb = graph(variant, params, W32), graph(variant, params, W16)
        assert ga.result.extra["w_path"] == "f32" and gb.result.extra["w_path"] == "u16"
        ra, rb = ga.launch(), gb.launch()
        torch.cuda.synchronize()
        same = all(torch.equal(getattr(ra, k), getattr(rb, k)) for k in ("Dn", "C", "I", "B_final", "B_hist"))
        if not same:
            raise SystemExit(f"{name}: uint16 and fp32 outputs differ")
        t_end = time.perf_counter() + 1.0  # clock ramp (bench.py PREWARM_S)
        while time.perf_counter() < t_end:
            for _ in range(4):
                ga.launch()
                gb.launch()
            torch.cuda.synchronize()
        for _ in range(a.warmup):
            ga.launch()
            gb.launch()
        torch.cuda.synchronize()
        ta, tb = [], []
        ev = [torch.cuda.Event(enable_timing=True) for _ in range(3)]
        for _ in range(max(a.replays, 20)):
            ev[0].record()
            ga.launch()
            ev[1].record()
            gb.launch()
            ev[2].record()
            torch.cuda.synchronize()
            ta.append(ev[0].elapsed_time(ev[1]))
            tb.append(ev[1].elapsed_time(ev[2]))
        ph = {}
        po = {k: getattr(ra, k) for k in ("Dn", "C", "I", "B_final", "B_hist")}  # the f32 graph's buffers, done with
        for tag, W in (("f32", W32), ("u16", W16)):
            reps = []
            for _ in range(a.phase_reps + 1):
                buf: list = []
                engine.run(variant, params, W, S, want_hist=True, out=po, workspace=ws, phase_ms=buf)
                reps.append(buf)
            reps = reps[1:]  # the first direct run warms the non-graph launch path
            ph[tag] = {p: round(statistics.median(r[i] for r in reps), 4) for i, p in enumerate(engine.PHASES)}
        sa, sb = spread(ta), spread(tb)
        line["versions"][name] = {
            "f32": sa, "u16": sb, "outputs_bit_equal": same,
            "u16_minus_f32_median_ms": round(sb["median_ms"] - sa["median_ms"], 4),
            "f32_spread_ms": round(sa["max_ms"] - sa["min_ms"], 4),
            "phases_ms": ph,
        }
        ga.close()
        gb.close()
    print(json.dumps(line), flush=True)


if __name__ == "__main__":
    main()
