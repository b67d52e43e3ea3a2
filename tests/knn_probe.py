"""The GPU side of the neighbour-query cases (tests/knn_cases.py): knn_gpu_kr runs vgpu_roadmap_knn_range with a
case's own k, r and kmax between guard rows.  Run as a program it is the helper of
tests/test_gpu_knn_params.py::test_variants_equal_oracle: the index's kernel variants are chosen by environment
variables read once per process, so each setting runs here as a fresh child, which answers the cases of the
input .npz (save_inputs) in index mode and writes the lists to the output .npz (the parent compares them with
the oracle)."""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (os.path.join(ROOT, "mr-vamp_amd"), os.path.dirname(os.path.abspath(__file__))):
    if p not in sys.path:
        sys.path.insert(0, p)

GUARD = 4  # rows of nbr / dist and words of cnt after the last row
SENT_I = -0x5A5A5A5B  # 0xA5A5A5A5 as int32
SENT_F = -12345.0


def knn_gpu_kr(vamp, V, k, r, kmax, q_first, q_count, mode):
    """vgpu_roadmap_knn_range with the context's kNN method set to `mode` (1 brute force, 2 spatial index) and the
    caller's k [n], r [n], kmax; rows are indexed from q_first.  The outputs are prefilled with a sentinel and carry
    GUARD rows / words after the last row: those must come back untouched, and cnt <= kmax.  Returns
    (nbr [q_count, kmax] uint32, dist, cnt)."""
    import torch
    from vamp_amd._lib import check, load
    n, dim = V.shape
    assert 1 <= q_count and q_first + q_count <= n and len(k) == n and len(r) == n
    dev = torch.device("cuda", 0)
    # np.array copies: the cases' arrays are read-only, which torch.from_numpy does not take
    tV = torch.from_numpy(np.array(V, np.float32)).to(dev)
    tk = torch.from_numpy(np.array(k, np.uint32).view(np.int32)).to(dev)
    tr = torch.from_numpy(np.array(r, np.float32)).to(dev)
    nbr = torch.full((q_count + GUARD, kmax), SENT_I, dtype=torch.int32, device=dev)
    dist = torch.full((q_count + GUARD, kmax), SENT_F, dtype=torch.float32, device=dev)
    cnt = torch.full((q_count + GUARD,), SENT_I, dtype=torch.int32, device=dev)
    ctx = vamp.context(0)
    ctx.set_stream(torch.cuda.current_stream(dev).cuda_stream)
    check(load().vgpu_set_knn_mode(ctx.h, mode), ctx.h)
    try:
        check(load().vgpu_roadmap_knn_range(ctx.h, dim, tV.data_ptr(), n, q_first, q_count, tk.data_ptr(),
                                            tr.data_ptr(), kmax, nbr.data_ptr(), dist.data_ptr(), cnt.data_ptr()),
              ctx.h)
        torch.cuda.synchronize()
    finally:
        load().vgpu_set_knn_mode(ctx.h, 0)
    nbr, dist, cnt = nbr.cpu().numpy(), dist.cpu().numpy(), cnt.cpu().numpy()
    assert (nbr[q_count:] == SENT_I).all(), "nbr written past the last row"
    assert (dist[q_count:] == np.float32(SENT_F)).all(), "dist written past the last row"
    assert (cnt[q_count:] == SENT_I).all(), "cnt written past the last row"
    cnt = cnt[:q_count].view(np.uint32)
    assert cnt.max() <= kmax, f"cnt {int(cnt.max())} above kmax {kmax}"
    return nbr[:q_count].view(np.uint32), dist[:q_count], cnt


def run_case(vamp, case, mode):
    """every range of the case: [(nbr, dist, cnt)]"""
    return [knn_gpu_kr(vamp, case.V, case.k, case.r, case.kmax, qf, qc, mode) for qf, qc in case.ranges]


def save_inputs(path, cases):
    """the cases' inputs for a child: <name>/V, k, r, kmax, ranges"""
    res = {}
    for c in cases:
        res[f"{c.name}/V"], res[f"{c.name}/k"], res[f"{c.name}/r"] = c.V, c.k, c.r
        res[f"{c.name}/kmax"] = np.int64(c.kmax)
        res[f"{c.name}/ranges"] = np.asarray(c.ranges, np.int64).reshape(-1, 2)
    np.savez(path, **res)


def main(inp, out):
    import vamp_amd
    z = np.load(inp, allow_pickle=False)
    res = {}
    for name in sorted({f.split("/")[0] for f in z.files}):
        V, k, r, kmax = z[f"{name}/V"], z[f"{name}/k"], z[f"{name}/r"], int(z[f"{name}/kmax"])
        for i, (qf, qc) in enumerate(z[f"{name}/ranges"].tolist()):
            nbr, dist, cnt = knn_gpu_kr(vamp_amd, V, k, r, kmax, qf, qc, 2)
            res[f"{name}/{i}/nbr"], res[f"{name}/{i}/dist"], res[f"{name}/{i}/cnt"] = nbr, dist, cnt
    np.savez(out, **res)


if __name__ == "__main__":
    main(sys.argv[1], sys.argv[2])
