"""Weight pairs to the dense uint16 W at the headline shape: the device call
against what a user does without it, one process, one build.

rows = 1000 * 256, M = 4096 (bench.py's c2 as E * V rows). Per pair density
(share of a row's columns that a pair names; default 1 %, 10 %, 100 %) the
lists are generated on the device: k = round(density * M) pairs per row at
distinct columns (a seeded start per row, then a fixed step), weights uniform
over 1..65535.

Device: engine.weights_from_pairs captured once per form into a graph and
replayed, a device-event time per replay, reported as min / median / max:
raw with status, raw without status (no read-back launch), upscale with status.
Density 0 (no pairs) is timed as well: the fill and two walks over empty rows,
the nearest this tool comes to the fill alone; W's bytes over that time is a
lower bound of the fill's store rate, to set beside tools/copybw's write-only
line from the same machine.

Host (once per density, wall clock): the lists are taken as CPU tensors; a
torch scatter on the CPU builds the dense tensor ("densify"), engine.to_u16
rescales it where asked (--host-upscale, one density: it is a float64 pass over
the dense tensor, the same work at every density), and the dense tensor is
copied host to device from pageable memory, ending in a synchronise. The
device result is compared with it bit for bit. Prints one JSON line.

    python tools/bench_pairs.py [--densities 0.01,0.1,1.0] [--replays 20] [--host-upscale 0.01] [--no-host]
    python tools/bench_pairs.py --profile 0.1   a few direct calls at one density and nothing else: the command a
                                                rocprofv3 --kernel-trace --stats pass wraps
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

from yuma_simulation._internal import engine  # noqa: E402

E, V, M = 1000, 256, 4096  # bench.py DEFAULTS["c2"], one scenario
SEED = 0x5EED0002


def spread(xs):
    return {"min_ms": round(min(xs), 4), "median_ms": round(statistics.median(xs), 4), "max_ms": round(max(xs), 4),
            "n": len(xs)}


def wrap16(x):
    """int32 values in [0, 65535] as torch.uint16 (through int16: torch has no uint16 arithmetic)."""
    return ((x + 32768) % 65536 - 32768).to(torch.int16).view(torch.uint16)


def lists(rows, density, dev, gen):
    k = int(round(density * M))
    row_ptr = torch.arange(rows + 1, dtype=torch.int64, device=dev) * k
    if k == 0:
        z = torch.empty(0, dtype=torch.uint16, device=dev)
        return row_ptr, z, z.clone(), k
    start = torch.randint(0, M, (rows, 1), dtype=torch.int32, device=dev, generator=gen)
    step = torch.arange(k, dtype=torch.int32, device=dev) * (M // k)  # k * (M // k) <= M: distinct columns
    uid = wrap16((start + step) % M).reshape(-1)
    del start
    val = torch.empty(rows * k, dtype=torch.uint16, device=dev)
    for a in range(0, rows * k, 1 << 27):  # (in slabs: the int32 intermediates of 10^9 pairs are large)
        n = min(1 << 27, rows * k - a)
        val[a:a + n] = wrap16(torch.randint(1, 65536, (n,), dtype=torch.int32, device=dev, generator=gen))
    return row_ptr, uid, val, k


def time_graph(fn, replays, warmup):
    fn()  # code objects loaded before the capture
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g, stream=torch.cuda.Stream()):
        fn()
    t_end = time.perf_counter() + 0.5  # clock ramp
    while time.perf_counter() < t_end:
        g.replay()
        torch.cuda.synchronize()
    for _ in range(warmup):
        g.replay()
    torch.cuda.synchronize()
    ts = []
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    for _ in range(replays):
        a.record()
        g.replay()
        b.record()
        torch.cuda.synchronize()
        ts.append(a.elapsed_time(b))
    return spread(ts)


def host_path(row_ptr, uid, val, rows, upscale):
    """What a user does without the call, timed step by step (seconds, wall clock)."""
    out = {}
    t0 = time.perf_counter()
    counts = row_ptr[1:] - row_ptr[:-1]
    r = torch.repeat_interleave(torch.arange(rows, dtype=torch.int64), counts)
    c = uid.view(torch.int16).to(torch.int64) & 0xFFFF
    W = torch.zeros(rows, M, dtype=torch.int16)
    W.index_put_((r, c), val.view(torch.int16))
    W = W.view(torch.uint16)
    del r, c
    out["densify_s"] = round(time.perf_counter() - t0, 3)
    if upscale:
        t0 = time.perf_counter()
        W = engine.to_u16(W)
        out["to_u16_s"] = round(time.perf_counter() - t0, 3)
    t0 = time.perf_counter()
    Wd = W.cuda()
    torch.cuda.synchronize()
    out["copy_h2d_s"] = round(time.perf_counter() - t0, 3)
    out["total_s"] = round(sum(out.values()), 3)
    return Wd, out


def main():
    ap = argparse.ArgumentParser(description=__doc__.splitlines()[0])
    ap.add_argument("--densities", default="0.01,0.1,1.0")
    ap.add_argument("--replays", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--epochs", type=int, default=E, help="rows = epochs * 256")
    ap.add_argument("--host-upscale", type=float, default=0.01, help="the density whose host path also runs to_u16")
    ap.add_argument("--no-host", action="store_true")
    ap.add_argument("--profile", type=float, default=None)
    a = ap.parse_args()
    dev = engine.device()
    rows = a.epochs * V
    gen = torch.Generator(device=dev)
    gen.manual_seed(SEED)
    W = torch.empty(rows, M, dtype=torch.uint16, device=dev)

    if a.profile is not None:
        row_ptr, uid, val, k = lists(rows, a.profile, dev, gen)
        for upscale in (False, True):
            for _ in range(4):
                engine.weights_from_pairs(row_ptr, uid, val, (rows, M), upscale=upscale, out=W)
        torch.cuda.synchronize()
        print(json.dumps({"profile": a.profile, "pairs_per_row": k, "engine_build_id": engine.build_id()}), flush=True)
        return

    line = {"tool": "bench_pairs", "shape": {"rows": rows, "M": M}, "w_bytes": rows * M * 2,
            "engine_build_id": engine.build_id(), "device": torch.cuda.get_device_name(dev),
            "launch": "hipGraph replay, one device-event time per replay", "densities": {}}
    row_ptr, uid, val, _ = lists(rows, 0.0, dev, gen)
    t = time_graph(lambda: engine.weights_from_pairs(row_ptr, uid, val, (rows, M), out=W, want_status=False),
                   a.replays, a.warmup)
    line["no_pairs"] = {"raw_no_status": t,
                        "fill_GBps_lower_bound": [round(rows * M * 2 / t[k] / 1e6) for k in ("max_ms", "median_ms",
                                                                                             "min_ms")]}
    for d in (float(x) for x in a.densities.split(",")):
        row_ptr, uid, val, k = lists(rows, d, dev, gen)
        call = lambda **kw: engine.weights_from_pairs(row_ptr, uid, val, (rows, M), out=W, **kw)  # noqa: E731
        rec = {"pairs_per_row": k, "nnz": rows * k, "list_bytes": rows * k * 4 + (rows + 1) * 8,
               "device": {"raw": time_graph(lambda: call(), a.replays, a.warmup),
                          "raw_no_status": time_graph(lambda: call(want_status=False), a.replays, a.warmup),
                          "upscale": time_graph(lambda: call(upscale=True), a.replays, a.warmup)}}
        if not a.no_host:
            t0 = time.perf_counter()
            h = [x.cpu() for x in (row_ptr, uid, val)]
            rec["lists_d2h_s"] = round(time.perf_counter() - t0, 3)  # (not part of the host path: a user has them there)
            for upscale in ((False, True) if d == a.host_upscale else (False,)):
                Wh, times = host_path(*h, rows, upscale)
                _, st = call(upscale=upscale)
                rec["host_upscale" if upscale else "host_raw"] = times
                rec["device_equals_host_" + ("upscale" if upscale else "raw")] = bool(torch.equal(W, Wh))
                rec["status_" + ("upscale" if upscale else "raw")] = engine.PairsStatus.from_tensor(st).__dict__
                del Wh
            del h
        line["densities"][str(d)] = rec
        print(json.dumps({str(d): rec}), file=sys.stderr, flush=True)  # progress, in case a later density is cut off
        del row_ptr, uid, val
    print(json.dumps(line), flush=True)


if __name__ == "__main__":
    main()
