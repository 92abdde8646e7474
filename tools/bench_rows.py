"""What a list of watched validator rows costs at the c2 shape, one process, one build.

The synthetic inputs are bench.py's c2 (same seed). Per version -- Yuma 3 and
Yuma 4 liquid alpha -- four graphs are built over the same inputs: the dense
fp32 bond history, no history, a row list of 8 validators and one of 64 (no
[V][M] history: the main run takes the history-less scan and k_bonds_rows
recomputes the watched rows). After a clock ramp and warm-up they are replayed
in turn (A, B, C, D, A, ...) with a device-event time per replay: each mode's
median and min-max in ms per 1000-epoch step, then the bond phase's HIP-event
time of a direct run of each (phase_ms; the row kernel is counted there). Every
watched history is compared bit for bit with the dense one's rows, and the
other outputs with the dense run's, before anything is timed. Exits non-zero
unless the 8-row step is shorter than the dense-history step. Prints one JSON
line and, with --log NAME, also writes it to profiles/rows/NAME.json.

    python tools/bench_rows.py [--replays 24] [--warmup 5] [--rows 8,64] [--ring-depth 8] [--log NAME]

--ring-depth only labels the line: the depth is the library's kRowsP (an A/B
build of another depth is picked with YUMA_LIB).
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
    ap.add_argument("--replays", type=int, default=24, help="timed replays per mode (>= 20)")
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--phase-reps", type=int, default=3)
    ap.add_argument("--rows", default="8,64", help="row-list lengths")
    ap.add_argument("--ring-depth", type=int, default=8, help="kRowsP of the library under test (a label)")
    ap.add_argument("--log", default=None, help="also write the line to profiles/rows/<log>.json")
    a = ap.parse_args()
    widths = [int(s) for s in a.rows.split(",")]
    dev = engine.device()
    W = engine.synth_weights(SEED, E, N, V, M)
    S = torch.from_numpy(synth.stakes(SEED, E, N, V)).to(dev)
    ws = torch.empty(engine.workspace_bytes(engine.VARIANT_YUMA4, N, E, V, M, False), dtype=torch.uint8, device=dev)
    # mode -> engine.run keywords
    modes = {"dense": dict(want_hist=True), "no_history": dict(want_hist=False)}
    rows = {}
    for n in widths:  # n rows spread over the validators, unsorted
        rows[n] = torch.tensor([(7 + k * (V // n) * 5) % V for k in range(n)], dtype=torch.int32, device=dev)
        modes[f"rows_{n}"] = dict(want_hist=False, watch_rows=rows[n])

    line = {"tool": "bench_rows", "shape": {"V": V, "M": M, "epochs": E, "scenarios": N},
            "engine_build_id": engine.build_id(), "launch": "hipGraph replay, modes in turn",
            "hist_bytes": {m: E * N * M * 4 * (V if kw["want_hist"] else len(kw["watch_rows"]) if "watch_rows" in kw else 0)
                           for m, kw in modes.items()},
            "ring_depth": a.ring_depth,
            "versions": {}}
    for name, variant, liquid in VERSIONS:
        params = [engine.make_params(variant, YumaConfig(yuma_params=YumaParams(liquid_alpha=liquid)))]
        graphs = {m: engine.RunGraph(variant, params, W, S, workspace=ws, **kw) for m, kw in modes.items()}
        res = {m: g.launch() for m, g in graphs.items()}
        torch.cuda.synchronize()
        dense = res["dense"]
        for m, r in res.items():
            ok = all(torch.equal(getattr(r, k), getattr(dense, k)) for k in ("Dn", "C", "I", "B_final"))
            if r.B_rows is not None:
                ok = ok and r.extra["rows_path"] == "native" and r.B_hist is None
                ok = ok and torch.equal(r.B_rows, dense.B_hist.index_select(2, modes[m]["watch_rows"].long()))
            if not ok:
                raise SystemExit(f"{name}: {m} differs from the dense run")
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
        line["versions"][name] = {"step": step, "bonds_phase_ms": bonds, "outputs_bit_equal": True}
        w0 = f"rows_{widths[0]}"
        line["versions"][name]["rows_below_dense"] = step[w0]["median_ms"] < step["dense"]["median_ms"]
        for g in graphs.values():
            g.close()
        del graphs, res, dense
        torch.cuda.empty_cache()
    print(json.dumps(line), flush=True)
    if a.log:
        os.makedirs(os.path.join(ROOT, "profiles", "rows"), exist_ok=True)
        with open(os.path.join(ROOT, "profiles", "rows", a.log + ".json"), "w") as f:
            f.write(json.dumps(line) + "\n")
    if not all(v["rows_below_dense"] for v in line["versions"].values()):
        raise SystemExit(f"the rows_{widths[0]} step is not shorter than the dense-history step")


if __name__ == "__main__":
    main()
