#!/usr/bin/env python3
"""Time of the pair matrices (dskgpu_colors_pairs) beside dskgpu_colors_rows on the same matrix in the same process.

Counts a workload (default c2_10Mx150, k = 31, abundance_min = 3) in FOUR contexts of one process, which the library's switches tell apart
(they are read when a context is created):
  * default      the shipped choice: k_color_pairs_reg up to CP_REG_SWITCH colours, k_color_pairs_tile above;
  * reg          DSKGPU_PAIRS_REG_MAX=8: k_color_pairs_reg wherever it is built (up to 8 colours);
  * tile         DSKGPU_PAIRS_REG_MAX=0: k_color_pairs_tile at every width;
  * tile_noskip  the same with DSKGPU_PAIRS_NO_SKIP: all-zero rows are not stepped over.
For every bank count (default 1 .. 8, 16, 64) the first context colours the stream, cut behind record ends into banks of equal
record counts; its matrix goes to the others through dskgpu_colors_rows / dskgpu_colors_load (the counts are deterministic: the same rows).
Timed with device events on the stream the contexts run on, one warm-up call each, then --reps rounds that ALTERNATE between
  * colors_rows, counts only: the copy reads the same bytes (and writes as many) -- the memory floor;
  * colors_pairs with all three outputs, and with `shared` alone, in every context;
  * the same at --sparse-min-count (default 3), where most rows of a many-bank matrix have no cell left: what stepping over them is worth.
Every context must give the same matrices (asserted).  The medians and all values go into the one JSON line on stdout.
"""
import argparse
import json
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

VARIANTS = {"default": {}, "reg": {"DSKGPU_PAIRS_REG_MAX": "8"}, "tile": {"DSKGPU_PAIRS_REG_MAX": "0"},
            "tile_noskip": {"DSKGPU_PAIRS_REG_MAX": "0", "DSKGPU_PAIRS_NO_SKIP": "1"}}


def timed(stream, fn):
    import torch
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record(stream)
    r = fn()
    e1.record(stream)
    e1.synchronize()
    return e0.elapsed_time(e1), r


def summary(ms):
    med = statistics.median(ms)
    return {"ms_median": round(med, 3), "ms_all": [round(x, 3) for x in ms], "spread": round((max(ms) - min(ms)) / med, 4)}


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--workload", default="c2_10Mx150")
    ap.add_argument("--k", type=int, default=31)
    ap.add_argument("--abundance-min", type=int, default=3)
    ap.add_argument("--banks", default="1,2,3,4,5,6,7,8,16,64")
    ap.add_argument("--sparse-min-count", type=int, default=3)
    ap.add_argument("--reps", type=int, default=5)
    args = ap.parse_args()
    if args.reps < 5:
        ap.error("--reps must be >= 5")
    import torch
    if not torch.cuda.is_available():
        sys.exit("bench_color_pairs.py needs a HIP device: there is no CPU path to time")
    from dsk_amd import KmerCounter, synth, engine
    dev = torch.device("cuda", 0)
    reads, gl, nr, rl = synth.make_workload(args.workload, dev)
    n, p = reads.numel(), reads.data_ptr()
    nl = torch.nonzero(reads == 10).reshape(-1)
    torch.cuda.synchronize()
    stream = torch.cuda.Stream(dev)
    result = {"bench": "color_pairs", "library": os.path.basename(engine.library_path()), "workload": args.workload, "device": torch.cuda.get_device_name(0),
              "reads": nr, "read_len": rl, "stream_bytes": n, "k": args.k, "abundance_min": args.abundance_min, "sparse_min_count": args.sparse_min_count,
              "banks": {}}
    ctx = {}
    with torch.cuda.stream(stream):
        try:
            for name, env in VARIANTS.items():
                os.environ.update(env)
                try:
                    kc = KmerCounter(kmer_size=args.k, abundance_min=args.abundance_min, stream=stream.cuda_stream, timing=True)
                finally:
                    for key in env:
                        del os.environ[key]
                kc.set_reads_device(p, n)
                kc.count()
                ctx[name] = kc
            first = ctx["default"]
            n_rows = first.result_device()[2]
            result["rows"] = n_rows
            for nb in [int(x) for x in args.banks.split(",")]:
                ends = [int(nl[(i + 1) * nl.numel() // nb - 1].item()) + 1 for i in range(nb - 1)] + [n]
                first.colors_begin(nb)
                first.colors_add(p, n, ends)
                counts = torch.zeros((n_rows, nb), dtype=torch.int32, device=dev)
                out = torch.zeros((3, nb, nb), dtype=torch.int64, device=dev)
                torch.cuda.synchronize()
                first.colors_rows(1, counts.data_ptr(), 0)
                names = [v for v in VARIANTS if v != "reg" or nb <= 8]
                for v in names[1:]:
                    ctx[v].colors_load(counts.data_ptr(), nb)
                ptrs = [out[x].data_ptr() for x in range(3)]
                calls = {"colors_rows": lambda: first.colors_rows(1, counts.data_ptr(), 0)}
                want = {}
                for v in names:
                    for mc in (1, args.sparse_min_count):
                        calls["%s all mc%d" % (v, mc)] = lambda v=v, mc=mc: ctx[v].colors_pairs(mc, *ptrs)
                        calls["%s shared mc%d" % (v, mc)] = lambda v=v, mc=mc: ctx[v].colors_pairs(mc, ptrs[0], 0, 0)
                stats = {}
                for key, fn in calls.items():                                # warm-up, and every context gives the same sums
                    st = fn()
                    if key != "colors_rows":
                        kind = key.split(" ", 1)[1]
                        got = (out[:1] if "shared" in kind else out).clone()
                        assert kind not in want or (torch.equal(want[kind][0], got) and want[kind][1] == st), key
                        want.setdefault(kind, (got, st))
                        stats["mc%s" % kind.split("mc")[1]] = st
                ms = {key: [] for key in calls}
                for _ in range(args.reps):                                   # alternating
                    for key, fn in calls.items():
                        ms[key].append(timed(stream, fn)[0])
                floor = statistics.median(ms["colors_rows"])
                r = {"matrix_bytes": 4 * n_rows * nb, "stats": stats, "times": {}}
                for key, v in ms.items():
                    r["times"][key] = summary(v)
                    r["times"][key]["over_colors_rows"] = round(statistics.median(v) / floor, 3)
                result["banks"][str(nb)] = r
                del counts, out, want
        finally:
            for kc in ctx.values():
                kc.close()
    print(json.dumps(result))


if __name__ == "__main__":
    main()
