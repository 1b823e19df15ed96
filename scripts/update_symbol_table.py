"""Per-symbol table of a `rocprofv3 --kernel-trace --stats` run of `bench.py --steps K --warmup W` (one pass, one GPU):
calls, total ms, and -- for the update-GEMM symbols -- the algorithmic flops each carried, split by the role of the
launch: (a) next block column, (b) rest of the trailing update, panel-internal update (panel_rec).

    python scripts/update_symbol_table.py TRACE_kernel_trace.csv [--size 65536 --ntest 4096]

The trace does not carry K or the role, so the launches of the factorisation are restated here (cholesky_inplace,
panel_rec and gemm_route for the default options: block 2048 from 32768 columns, lookahead, 128-column leaves) and laid
over the trace symbol by symbol in start order; a symbol whose number of calls differs from the restated one is
reported as unmatched instead of being split.  Flops: 2K per element on or below the diagonal, real rows only
(gpmi_plan.h: plan_algorithmic_flops)."""
import argparse
import collections
import csv

TALL_TRAIL, DMA_TRAIL = "chol_trailing_update_dma256_kernel", "chol_trailing_update_dma_kernel"
TALL, DMA = "gemm_nt_dma_tall_kernel<false>", "gemm_nt_dma_kernel<2, false>"


def live_tiles(Tm, Tn):
    return sum(min(Tn, ti + 1) for ti in range(Tm))


def flops(M, N, K, real_rows):
    rows = min(M, real_rows)
    tri = min(rows, N - 1)
    return 2.0 * K * (tri * (tri + 1) / 2.0 + max(0, rows - tri) * N)


def launches(ncols, nrows, carried, tall_min=12288, tall_min_slack=1024):
    """(symbol, role, flops) of every LDS-DMA-family update launch of one factorisation, per stream in issue order"""
    nb = 2048 if ncols >= 32768 else 1024 if ncols >= 12288 else 512
    bar = tall_min_slack if ncols >= 49152 else tall_min
    out = []

    def gemm(role, counted, r0, M, N, K):
        Tm, Tn = M // 128, N // 128
        if Tm * Tn < 128:
            return
        tall = live_tiles(Tm, Tn) >= bar
        sym = (TALL_TRAIL if tall else DMA_TRAIL) if counted else (TALL if tall else DMA)
        out.append((sym, role, flops(M, N, K, ncols - r0 + 1 + carried)))

    def panel(k, off, w):
        if w <= 128:
            return
        h = w // 2 // 128 * 128
        panel(k, off, h)
        gemm("panel", False, k + off + h, nrows - k - off - h, w - h, h)
        panel(k, off + h, w - h)

    for k in range(0, ncols, nb):
        panel(k, 0, nb)
        r0 = k + nb
        if r0 >= ncols:
            break
        gemm("(a)", False, r0, nrows - r0, nb, nb)
        if r0 + nb < ncols:
            gemm("(b)", True, r0 + nb, nrows - r0 - nb, ncols - r0 - nb, nb)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("trace")
    ap.add_argument("--size", type=int, default=65536)
    ap.add_argument("--ntest", type=int, default=4096)
    args = ap.parse_args()
    rows = list(csv.DictReader(open(args.trace)))
    rows.sort(key=lambda r: int(r["Start_Timestamp"]))
    by_sym = collections.OrderedDict()
    for r in rows:
        name = r["Kernel_Name"].replace("void ", "").replace("gpmi::", "").split("(")[0]
        by_sym.setdefault(name, []).append((int(r["End_Timestamp"]) - int(r["Start_Timestamp"])) * 1e-6)
    ncols = (args.size + 127) // 128 * 128
    model = launches(ncols, ncols + 128 + args.ntest, args.ntest)
    per_sym = collections.defaultdict(list)
    for sym, role, f in model:
        per_sym[sym].append((role, f))
    upd = (TALL_TRAIL, DMA_TRAIL, TALL, DMA)
    upd_ms = sum(sum(by_sym.get(s, [])) for s in upd)
    print("%-44s %-8s %6s %10s %7s %10s %7s" % ("symbol", "role", "calls", "ms", "% upd", "Tflop", "% flop"))
    table, tot_f = [], 0.0
    for sym, ms in sorted(by_sym.items(), key=lambda kv: -sum(kv[1])):
        want = per_sym.get(sym)
        if sym in upd and want and len(ms) % len(want) == 0:
            acc = collections.OrderedDict()
            for i, t in enumerate(ms):
                role, f = want[i % len(want)]
                a = acc.setdefault(role, [0, 0.0, 0.0])
                a[0] += 1; a[1] += t; a[2] += f
            for role, (n, t, f) in acc.items():
                table.append((sym, role, n, t, f)); tot_f += f
        else:
            table.append((sym, "unmatched" if sym in upd else "", len(ms), sum(ms), None))
    for sym, role, n, t, f in table:
        print("%-44s %-8s %6d %10.2f %7s %10s %7s" % (sym, role, n, t, "%.1f" % (100 * t / upd_ms) if sym in upd else "",
                                                       "%.2f" % (f * 1e-12) if f is not None else "",
                                                       "%.1f" % (100 * f / tot_f) if f is not None else ""))
    small = sum(t for s, _, _, t, _ in table if s in (DMA_TRAIL, DMA))
    print("update symbols: %.2f ms summed over the launches; 128 x 128 symbols %.2f ms = %.1f %%" % (upd_ms, small, 100 * small / upd_ms))


if __name__ == "__main__":
    main()
