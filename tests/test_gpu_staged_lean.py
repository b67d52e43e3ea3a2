"""The bookkeeping of a staged pass (vgpu_api.cpp staged_pass, vgpu_kernels.hip staged_scan_kernel): the per-check scan with its carried prefix, the plan laid out by the scan's last block,
the totals that block stores into pinned memory, the item total summed by the tail_counts kernels
(vgpu_lean.hh item_total_block), and the ticket words and accumulators the kernels reset themselves.  Every result is compared with the oracle's (same host: bit for bit).

The scan works in tiles of 1024 per-(check, block) counts and a block of the count stage covers 256 groups, so
262,145 edges is the smallest batch whose head pass carries a prefix from one tile into the next (a 256-entry
tile would put that at 70,001 edges or fewer); the tails of that batch run over several tiles."""
import os
import sys

import numpy as np
import pytest

from test_gpu_parity import gpu_env_from_oracle
from test_oracle_fetch import fetch_env
from conftest import host_fixture

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import bench  # noqa: E402

pytestmark = pytest.mark.gpu
F = np.float32
_KEEP = []  # contexts stay alive as long as the environments that hold copies on them
TILE_EDGES = 1024 * 256 + 1  # nb = 1025 blocks of 256 groups: the second scan tile holds one count


@pytest.fixture(scope="module")
def vamp():
    import vamp_amd
    assert vamp_amd.context(0) is not None
    return vamp_amd


@pytest.fixture(scope="module")
def cage(vamp, oracle):
    oenv = oracle.sphere_cage_env()
    return oenv, gpu_env_from_oracle(vamp, oenv)


@pytest.fixture(scope="module")
def pool(vamp, oracle, cage):
    """TILE_EDGES cage edges: three quarters drawn as bench.make_edges draws set B (valid endpoints, length
    capped at 1), one quarter raw set-A pairs, shuffled; with the oracle's results, computed once."""
    import torch
    oenv, env = cage
    dev = torch.device("cuda", 0)
    n_a = TILE_EDGES // 4
    sb, gb = bench.make_edges(torch, vamp, env, vamp.panda_0_0, TILE_EDGES - n_a, 7, dev, "B")
    sa, ga = bench.make_edges(torch, vamp, env, vamp.panda_0_0, n_a, 8, dev, "A")
    s = torch.cat([sb, sa]).cpu().numpy()
    g = torch.cat([gb, ga]).cpu().numpy()
    perm = np.random.default_rng(9).permutation(TILE_EDGES)
    s, g = np.ascontiguousarray(s[perm]), np.ascontiguousarray(g[perm])
    ok, n = oracle.validate_motions(oenv, s, g, (0, 0, 0))
    for a in (s, g, ok, n):
        a.setflags(write=False)
    return s, g, ok, n


@pytest.mark.parametrize("n_edges", [1, 255, 256, 257, TILE_EDGES])
def test_panda_validate_cage(vamp, cage, pool, n_edges):
    s, g, rok, rn = pool
    ok, n = vamp.panda_0_0.validate_batch(s[:n_edges], g[:n_edges], cage[1])
    assert np.array_equal(n, rn[:n_edges])
    assert np.array_equal(ok, rok[:n_edges])
    if n_edges == TILE_EDGES:
        assert 0.05 < ok.mean() < 0.95 and (n[ok != 0] > 1).any()  # heads, tails and survivors all exercised


def test_empty_environment(vamp, oracle, pool, capfd):
    """No obstacle: every environment check's total is 0 in every pass (read from the passes' statistics lines,
    VAMP_AMD_STAGED_STATS), so no environment children launch -- their grids are sized from those totals; the
    self checks still bound and run, and the results equal the oracle's."""
    import ctypes as C
    from vamp_amd._lib import load
    s, g = pool[0][:4099], pool[1][:4099]
    rok, rn = oracle.validate_motions(oracle.Env(), s, g, (0, 0, 0))
    os.environ["VAMP_AMD_STAGED_STATS"] = "1"
    try:
        ctx = vamp.Context(0)  # reads VAMP_AMD_STAGED_STATS at creation
    finally:
        del os.environ["VAMP_AMD_STAGED_STATS"]
    env = vamp.Environment()
    _KEEP.extend([ctx, env])
    capfd.readouterr()
    ok, n = vamp.panda_0_0.validate_batch(s, g, env, ctx)
    lines = [ln for ln in capfd.readouterr().err.splitlines() if ln.startswith("staged kind=")]
    fn = load().vgpu_panda_p0_staged_env_checks
    fn.restype = C.c_uint64
    env_bits = int(fn())
    assert env_bits and {ln.split()[1] for ln in lines} == {"kind=2", "kind=3"}  # a head and a tail pass
    for ln in lines:
        fired = [int(x) for x in ln.split("fired:")[1].split()]
        assert len(fired) == 32 and sum(fired) > 0
        assert all(f == 0 for k, f in enumerate(fired) if (env_bits >> k) & 1), ln
    assert np.array_equal(n, rn) and np.array_equal(ok, rok)
    assert ok.mean() > 0.5


def test_every_head_invalid(vamp, oracle, cage, pool):
    """One sphere over the robot's base: every first block collides, so the item total is 0 and no tail pass
    runs; the context serves the next call as usual."""
    s, g, rok, rn = pool
    oenv = oracle.Env()
    oenv.add_sphere(np.array([0, 0, 0.3], F), F(0.6))
    env = gpu_env_from_oracle(vamp, oenv)
    ok, n = vamp.panda_0_0.validate_batch(s[:4099], g[:4099], env)
    assert not ok.any() and np.array_equal(n, rn[:4099])
    ok2, n2 = vamp.panda_0_0.validate_batch(s[:4099], g[:4099], cage[1])
    assert np.array_equal(ok2, rok[:4099]) and np.array_equal(n2, rn[:4099])


@pytest.mark.parametrize("n_edges", [257, 4099])
def test_fetch_validate(vamp, oracle, n_edges):
    """64-bit check masks, 63 checks (one scan block per check)."""
    fx = host_fixture("fetch_table_pick.npz", oracle)
    oenv = fetch_env(oracle, fx)
    env = gpu_env_from_oracle(vamp, oenv)
    rng = np.random.default_rng(100 + n_edges)
    s = oracle.robot_scale("fetch", rng.random((n_edges, 8), dtype=F))
    g = oracle.robot_scale("fetch", rng.random((n_edges, 8), dtype=F))
    g[::2] = s[::2] + (g[::2] - s[::2]) * F(0.1)
    ok, n = vamp.fetch.validate_batch(s, g, env)
    rok, rn = oracle.robot_validate_motions("fetch", oenv, s, g)
    assert np.array_equal(n, rn) and np.array_equal(ok, rok)
    assert 0 < ok.sum() < n_edges


@pytest.mark.parametrize("n_edges", [257, 4099])
def test_pair_validate(vamp, oracle, n_edges):
    """The two-Panda composite: four chained passes per stage, each with its own scan, plan and read-back."""
    oenv = oracle.pair_scene()
    env = gpu_env_from_oracle(vamp, oenv)
    rng = np.random.default_rng(200 + n_edges)
    u = rng.random((2 * n_edges, 14), dtype=F)
    q = np.concatenate([oracle.scale(u[:, :7]), oracle.scale(u[:, 7:])], 1)
    s, g = q[:n_edges], q[n_edges:].copy()
    g[::2] = s[::2] + (g[::2] - s[::2]) * F(0.15)
    ok, n = vamp.panda_pair.validate_batch(s, g, env)
    rok, rn = oracle.pair_validate_motions(oenv, s, g, (0, 0, 0), (100, 0, 0))
    assert np.array_equal(n, rn) and np.array_equal(ok, rok)
    assert 0 < ok.sum() < n_edges


@pytest.mark.parametrize("n_q", [65, 16385])
def test_fkcc_configurations(vamp, oracle, cage, n_q):
    """Source kind 0 (64 groups per wave): rounds picked on the host, so the first round keeps plan_kernel."""
    q = oracle.scale(np.random.default_rng(300 + n_q).random((n_q, 7), dtype=F))
    got = vamp.panda_0_0.fkcc_batch(q, cage[1])
    assert np.array_equal(got, oracle.fkcc_threads(cage[0], q, (0, 0, 0)))
    assert 0 < got.sum() < n_q


def test_early_exit_guard(vamp, oracle, cage):
    """validate_device rejects a batch of more than 2^32 rake blocks before any offset is used, and the item
    total's accumulator and ticket are back at zero for the next call.

    The three saturating edges of test_too_many_blocks_rejected cannot reach the guard in early-exit mode, in
    any build: their start self-collides (joint 4 at -1.5, the rest 0) and joint 1 beyond ~1e4 rad is outside the
    FK's sine range, so their head block is invalid and no back-step is counted -- they come back invalid.  The
    guard is reached with 220,000 copies of an edge whose head block is valid and which has 20,000 blocks."""
    import torch
    dev = torch.device("cuda", 0)
    ctx = vamp.context(0)
    empty = vamp.Environment()

    def run(s, g):
        n = s.shape[0]
        ds, dg = torch.from_numpy(s).to(dev), torch.from_numpy(g).to(dev)
        ok = torch.empty(n, dtype=torch.uint8, device=dev)
        nb = torch.empty(n, dtype=torch.int32, device=dev)
        vamp.panda_0_0.validate_device(ds.data_ptr(), dg.data_ptr(), n, empty, ok.data_ptr(), nb.data_ptr(), ctx)
        ctx.sync()
        return ok.cpu().numpy(), nb.cpu().numpy()

    s = np.zeros((3, 7), F)
    s[:, 3] = -1.5
    g = s.copy()
    g[:, 0] += F(1e9)
    ok, nb = run(s, g)
    assert not ok.any() and (nb == 2147483520).all()
    home = np.array([0, -0.785, 0, -2.356, 0, 1.571, 0.785], F)
    far = home.copy()
    far[0] += F(5000)
    head = np.stack([home + (far - home) * F((i + 1) / 8) for i in range(8)]).astype(F)
    assert oracle.fkcc_threads(oracle.Env(), head, (0, 0, 0)).all()
    _, n1 = run(home[None], far[None])
    n_edges = 220000
    assert n_edges * int(n1[0]) >= 1 << 32 and int(n1[0]) == 20000
    with pytest.raises(vamp.VgpuError, match="2\\^32"):
        run(np.tile(home, (n_edges, 1)), np.tile(far, (n_edges, 1)))
    ctx.sync()
    rng = np.random.default_rng(5)
    a = oracle.scale(rng.random((300, 7), dtype=F))
    b = (a + (oracle.scale(rng.random((300, 7), dtype=F)) - a) * F(0.2)).astype(F)
    got = vamp.panda_0_0.validate_batch(a, b, cage[1])
    ref = oracle.validate_motions(cage[0], a, b, (0, 0, 0))
    assert np.array_equal(got[0], ref[0]) and np.array_equal(got[1], ref[1])


def test_repeatable_on_one_context(vamp, oracle, cage, pool):
    """Large then small on one context equals a fresh context's results: tickets, accumulators and the pinned
    totals carry nothing from call to call."""
    s, g, rok, rn = pool
    env = gpu_env_from_oracle(vamp, cage[0])
    one, fresh = vamp.Context(0), vamp.Context(0)
    _KEEP.extend([one, fresh, env])
    big = vamp.panda_0_0.validate_batch(s[:70001], g[:70001], env, one)
    small = vamp.panda_0_0.validate_batch(s[:300], g[:300], env, one)
    small_fresh = vamp.panda_0_0.validate_batch(s[:300], g[:300], env, fresh)
    assert np.array_equal(big[0], rok[:70001]) and np.array_equal(big[1], rn[:70001])
    assert np.array_equal(small[0], small_fresh[0]) and np.array_equal(small[1], small_fresh[1])
    assert np.array_equal(small[0], rok[:300]) and np.array_equal(small[1], rn[:300])
