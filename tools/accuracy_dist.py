"""Worst error of the distributed transform's two phases per case, world and rank, over the CASES of
tests/test_gpu_dist_elementwise.py and three seeds: the evidence behind K_PRE and K_DIST of tests/elementwise_bound.py and
behind using the kernel matrix's K_SINCOS unchanged for distributed plans with a sin / cos kernel.

Send buffer (after tfft_dist_exec_pre): binary16 ulps of each column's largest bin. Output (after tfft_dist_exec_post): ulps of the
largest bin of the whole N-point spectrum. Each case runs with every assertion of the test module and K = 4 (the ceiling the K
values may not exceed), so that a case above a committed K is measured rather than stopped. Writes profiles/dist_ulps.txt (or the
path given); --lg restricts the lengths (one part of the cases per run, the parts' files joined by hand into the profile),
--seeds the seeds.

    python tools/accuracy_dist.py [--lg 15,16,20] [--seeds 1,2,3] [out.txt]
"""
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]


def k_rule(worst):
    return min(4.0, max(0.5, -(-1.5 * worst // 0.5) * 0.5))


def main():
    import torch

    import __graft_entry__ as g

    g.build()
    import elementwise_bound as eb
    import test_gpu_dist_elementwise as td
    import tensor_fft_amd as tf
    from tensor_fft_amd import capi
    from test_gpu_kernel_matrix import arithmetic_class

    args, lgs, seeds = sys.argv[1:], None, (1, 2, 3)
    if "--lg" in args:
        i = args.index("--lg")
        lgs = {int(v) for v in args[i + 1].split(",")}
        del args[i:i + 2]
    if "--seeds" in args:
        i = args.index("--seeds")
        seeds = tuple(int(v) for v in args[i + 1].split(","))
        del args[i:i + 2]
    out = args[0] if args else os.path.join(ROOT, "profiles", "dist_ulps.txt")
    tf.device_check(0)
    lines, send_worst, out_worst = [], 0.0, {}
    cases = [c for c in td.CASES if lgs is None or c[0] in lgs]
    for lg in sorted({c[0] for c in cases}):
        for seed in seeds:
            signal = td.make_signal(lg, seed)
            for _, world, slabs in [c for c in cases if c[0] == lg]:
                t0 = time.time()
                res, (pre, post) = td.run_case(torch, capi, lg, world, slabs, signal, seed=seed, k_pre=4.0, k_out=4.0)
                cls = arithmetic_class(pre + post, {"kind": "c"})
                for rank, w_send, w_out, rel, _ in res:
                    lines.append(f"{lg:3d} {world:3d} {slabs:2d} {seed:2d} {rank:3d}  {w_send:6.3f}  {w_out:6.3f}  {rel:9.3e}  {cls}")
                    send_worst = max(send_worst, w_send)
                    out_worst[cls] = max(out_worst.get(cls, 0.0), w_out)
                print(f"2^{lg} x {world} ranks, {slabs} slab(s), seed {seed}: done in {time.time() - t0:.0f} s", flush=True)
            del signal
    with open(out, "w") as f:
        f.write("# tools/accuracy_dist.py: worst max(|dRe|, |dIm|) of the two phases of a distributed transform, all ranks in one process\n")
        f.write("# (tests/dist_emulate.py), over tests/test_gpu_dist_elementwise.py CASES. send: the send buffer after pre against fp64, in binary16\n")
        f.write("# ulps of each column's largest bin; out: the output after post, in ulps of the largest bin of the whole spectrum (2^28 and\n")
        f.write("# 2^29: of the sampled rows); rel-L2 of the rank's share (of its sampled rows). One MI355X.\n")
        f.write("# lg world slabs seed rank   send     out    rel-L2    class\n")
        f.write("\n".join(lines) + "\n")
        f.write(f"# class worst send    {send_worst:6.3f} ulp -> K_PRE = {min(k_rule(send_worst), eb.K_TABLE):.1f} (smallest half-integer >= 1.5 x worst, at most K_TABLE)\n")
        kernel_matrix = {"table": 1.84, "sincos": 1.64}          # profiles/per_kernel_ulps.txt, class worst
        for cls, w in sorted(out_worst.items()):
            verdict = (f"<= {kernel_matrix[cls]} of profiles/per_kernel_ulps.txt: K_{cls.upper()} unchanged" if w <= kernel_matrix[cls]
                       else f"> {kernel_matrix[cls]} of profiles/per_kernel_ulps.txt -> K_DIST = {k_rule(w):.1f}")
            f.write(f"# class worst output {cls:7s} {w:6.3f} ulp, {verdict}\n")
    print(open(out).read())


if __name__ == "__main__":
    main()
