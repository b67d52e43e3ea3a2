"""The clearance grid (vgpu_clear_grid.hip, vgpu_device.hh clear_lane): per cell a lower bound of the distance to
the nearest obstacle surface; the Panda's validate bound kernels skip the obstacle scans of bounding spheres it
proves clear.  It must change no result, so the oracle (oracle_py) is the checker throughout, bitwise on ok and
n_e:

* the grid itself against a float64 restatement of its formula: never above the exact bound (soundness), never
  more than two quantisation steps below it (tightness: an all-zero grid fails);
* motions with the grid on: partial waves, block boundaries, many blocks; the robot inside the grid's box, far
  outside it (base 200, 200, 0), and a scene of cuboids that fills part of the workspace (table_pick);
* obstacles placed at a robot sphere's surface +- epsilon, with epsilon around the float rounding, the grid's
  margin and a cell's diagonal;
* environments that must get no grid (sheared cuboid, heightfield, one record past the cap, a NaN coordinate,
  no obstacle): still the oracle's results;
* an obstacle added after the first call (a stale grid would pass the first call and fail the second);
* VAMP_AMD_CLEAR=0 in a child process: identical results.
"""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

from clear_probe import clear_batch
from test_gpu_parity import gpu_env_from_oracle

F = np.float32
HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
CAP = 256  # vgpu_device.hh kClrMaxRecords


@pytest.fixture(scope="module")
def vamp():
    import vamp_amd
    assert vamp_amd.context(0) is not None
    return vamp_amd


def unit(v):
    return v / np.linalg.norm(v)


def rotation(rng):
    Q, _ = np.linalg.qr(rng.normal(size=(3, 3)))
    return Q


# ---- 1. the grid against its formula --------------------------------------------------------------------------
def grid_scenes(oracle):
    rng = np.random.default_rng(3)
    mixed = oracle.Env()
    mixed.add_capsule_endpoints([0.4, -0.3, 0.2], [0.1, 0.5, 0.9], F(0.07))
    R = rotation(rng)
    mixed.add_cuboid_axes([-0.4, 0.3, 0.5], R[:, 0].astype(F), R[:, 1].astype(F), R[:, 2].astype(F), [0.1, 0.2, 0.05])
    a = 0.7
    mixed.add_cuboid_axes([0.5, 0.5, 0.1], np.array([np.cos(a), np.sin(a), 0], F),
                          np.array([-np.sin(a), np.cos(a), 0], F), np.array([0, 0, 1], F), [0.2, 0.1, 0.1])
    assert len(mixed.capsules) == 1 and len(mixed.cuboids) == 1 and len(mixed.zcuboids) == 1
    tiny = oracle.Env().add_sphere([0.3, 0.2, 0.5], F(1e-3))
    far = oracle.Env().add_sphere([-500.0, 0.0, 0.5], F(0.3)).add_sphere([500.0, 0.2, 0.4], F(0.3))
    far.add_capsule_endpoints([0.0, 400.0, 0.0], [0.0, 400.0, 2.0], F(0.1))
    return {"cage": oracle.sphere_cage_env(), "mixed": mixed, "tiny_sphere": tiny, "far_apart": far}


def exact_distance(oenv, p):
    """float64 distance from the points p[..., 3] to the nearest record's surface (0 inside a cuboid)"""
    d = np.full(p.shape[:-1], np.inf)
    for x, y, z, r, _ in oenv.spheres:
        d = np.minimum(d, np.linalg.norm(p - np.array([x, y, z], np.float64), axis=-1) - float(r))
    for row in oenv.capsules + oenv.zcapsules:
        row = np.array(row, np.float64)
        p1, v, r = row[0:3], row[3:6], row[6]
        t = np.clip(((p - p1) @ v) / (v @ v), 0.0, 1.0)
        d = np.minimum(d, np.linalg.norm(p - (p1 + t[..., None] * v), axis=-1) - r)
    for row in oenv.cuboids + oenv.zcuboids:
        row = np.array(row, np.float64)
        c, A, h = row[0:3], row[3:12].reshape(3, 3), row[12:15]
        a = np.maximum(np.abs((p - c) @ A.T) - h, 0.0)
        d = np.minimum(d, np.linalg.norm(a, axis=-1))
    return d


@pytest.mark.gpu
@pytest.mark.parametrize("name", ["cage", "mixed", "tiny_sphere", "far_apart"])
def test_grid_is_sound_and_tight(vamp, oracle, name):
    oenv = grid_scenes(oracle)[name]
    env = gpu_env_from_oracle(vamp, oenv)
    hdr, cells = env.clear_grid()
    assert hdr is not None, "this environment must have a clearance grid"
    N, step = hdr["n"], float(hdr["step"])
    lo, h = hdr["lo"].astype(np.float64), hdr["h"].astype(np.float64)
    assert N in (64, 128) and (h > 0).all() and abs(step - 1.0 / 512.0) < 1e-12
    assert np.allclose(hdr["inv_h"].astype(np.float64) * h, 1.0, rtol=1e-6)
    # every record lies inside A, and the grid's box contains A with a pad of at least 0.3 m
    assert (lo <= hdr["a_lo"] - 0.3 + 1e-4).all() and (lo + N * h >= hdr["a_hi"] + 0.3 - 1e-4).all()
    extent = float((N * h).max())
    assert float(hdr["margin"]) >= 1e-3 + 1e-5 * extent * (1 - 1e-3)
    idx = (np.arange(N) + 0.5)
    Z, Y, X = np.meshgrid(idx, idx, idx, indexing="ij")  # cells[iz, iy, ix]
    p = np.stack([lo[0] + X * h[0], lo[1] + Y * h[1], lo[2] + Z * h[2]], axis=-1)
    bound = exact_distance(oenv, p) - 0.5 * np.linalg.norm(h) - float(hdr["margin"])
    dev = cells.astype(np.float64) * step
    print(f"clear grid {name}: N {N}, cell {h}, margin {float(hdr['margin']):.3g}, nonzero {np.mean(cells > 0):.3f}, "
          f"saturated {np.mean(cells == 255):.3f}, max dev - bound {np.max(dev - np.maximum(bound, 0)):.3g}, "
          f"max bound - dev {np.max(np.minimum(bound, 255 * step) - dev):.3g}", flush=True)
    assert (dev <= np.maximum(bound, 0.0)).all(), "a cell claims more clearance than the exact bound"
    assert (dev >= np.minimum(bound, 255 * step) - 2 * step).all(), "a cell is more than two steps below the bound"
    assert (cells > 0).any()
    a_lo, a_hi = hdr["a_lo"].astype(np.float64), hdr["a_hi"].astype(np.float64)
    for x, y, z, r, _ in oenv.spheres:  # A holds the records
        c = np.array([x, y, z], np.float64)
        assert (c - r >= a_lo - 1e-6).all() and (c + r <= a_hi + 1e-6).all()


# ---- 2. motions with the grid on ---------------------------------------------------------------------------------
def edges(oracle, n, seed):
    s, g = clear_batch(n, seed)
    s, g = oracle.scale(s), oracle.scale(g)
    g[::3] = oracle.scale(np.random.default_rng(seed + 1).random((len(g[::3]), 7), dtype=F))  # long edges too
    return s, g


@pytest.fixture(scope="module")
def scenes(vamp, oracle):
    from conftest import host_fixture
    from test_oracle_robots import scene_env
    out = {"cage": oracle.sphere_cage_env(), "table_pick": scene_env(oracle, host_fixture("panda_table_pick.npz", oracle))}
    return {k: (o, gpu_env_from_oracle(vamp, o)) for k, o in out.items()}


@pytest.mark.gpu
@pytest.mark.parametrize("n", [1, 7, 9, 33, 257, 4096])
@pytest.mark.parametrize("scene,base", [("cage", (0, 0, 0)), ("cage", (200, 200, 0)), ("table_pick", (0, 0, 0))])
def test_motions_equal_the_oracle(vamp, oracle, scenes, scene, base, n):
    oenv, env = scenes[scene]
    assert env.clear_grid()[0] is not None
    s, g = edges(oracle, n, 100 + n)
    ok, ne = vamp.PandaBase(*base).validate_batch(s, g, env)
    rok, rne = oracle.validate_motions(oenv, s, g, base)
    assert np.array_equal(ne, rne) and np.array_equal(ok, rok), (scene, base, n, int((ok != rok).sum()))


# ---- 3. obstacles at a robot sphere's surface +- epsilon -------------------------------------------------------
EPS = ["-1e-4", "-1e-6", "0", "+1e-6", "+1e-4", "margin*0.5", "margin*1.5", "cell_diagonal"]
N_GRAZE = 200


def panda_radii():
    m = json.load(open(os.path.join(ROOT, "model", "panda.json")))
    return np.array([s["radius"] for s in m["spheres"]], np.float64)


def graze_configs(oracle):
    rng = np.random.default_rng(808)
    q = oracle.scale(rng.random((4 * N_GRAZE, 7), dtype=F))
    q = q[oracle.fkcc_threads(oracle.Env(), q)][:N_GRAZE]
    assert len(q) == N_GRAZE
    return q, oracle.sphere_fk(q).astype(np.float64)


def graze_env(oracle, rng, c, r, eps, away):
    """one sphere, one capsule (end cap on its axis) and one cuboid (face contact; z-aligned for every other one),
    each at surface distance r + eps from c, in three directions 0.25 rad off `away` (out of the robot)"""
    e = oracle.Env()
    gap = r + eps
    u = unit(np.cross(away, rng.normal(size=3)))
    w = np.cross(away, u)
    ph = rng.uniform(0, 2 * np.pi)
    n = [unit(away * np.cos(0.25) + (u * np.cos(ph + k * 2.1) + w * np.sin(ph + k * 2.1)) * np.sin(0.25)) for k in range(3)]
    e.add_sphere((c + n[0] * (gap + 0.05)).astype(F), F(0.05))
    rc, L = rng.uniform(0.01, 0.1), rng.uniform(0.05, 0.5)
    e.add_capsule_endpoints(c + n[1] * (gap + rc), c + n[1] * (gap + rc + L), F(rc))
    h = rng.uniform(0.02, 0.06, 3)
    a1 = n[2]
    if rng.random() < 0.5 and np.hypot(a1[0], a1[1]) > 0.2:  # a z-cuboid: the contact normal in the xy plane
        a1 = unit(np.array([a1[0], a1[1], 0.0]))
        a3 = np.array([0.0, 0.0, 1.0])
    else:
        a3 = unit(np.cross(a1, rng.normal(size=3)))
    a2 = np.cross(a3, a1)
    e.add_cuboid_axes(c + a1 * (h[0] + gap), a1.astype(F), a2.astype(F), a3.astype(F), h.astype(F))
    return e


def graze_cases(oracle, eps_of):
    """[(oracle env, starts, goals)]: per configuration short edges ending at it; eps_of(env at eps 0) -> eps"""
    q, xyz = graze_configs(oracle)
    rads = panda_radii()
    rng = np.random.default_rng(4242)
    out = []
    for i in range(N_GRAZE):
        k = int(rng.integers(len(rads)))
        cand = rng.normal(size=(64, 3))  # the direction in which sphere k's surface is farthest from the others
        cand /= np.linalg.norm(cand, axis=1, keepdims=True)
        pts = xyz[i, k] + cand * rads[k]
        other = np.delete(np.arange(len(rads)), k)
        gapo = np.linalg.norm(pts[:, None] - xyz[i, other][None], axis=-1) - rads[other][None]
        away = cand[int(np.argmax(gapo.min(axis=1)))]
        eps = eps_of(lambda: graze_env(oracle, np.random.default_rng(i), xyz[i, k], rads[k], 0.0, away))
        e = graze_env(oracle, np.random.default_rng(i), xyz[i, k], rads[k], eps, away)
        s = (q[i][None] + rng.normal(scale=[[1e-4], [1e-3], [1e-2], [0.1]], size=(4, 7))).astype(F)
        out.append((e, s, np.repeat(q[i][None], 4, axis=0)))
    return out


def test_grazing_set_has_both_outcomes(oracle):
    """the oracle alone (no GPU): the fixed epsilons give colliding and free edges"""
    oks = []
    for eps in (-1e-4, -1e-6, 0.0, 1e-6, 1e-4):
        ok = np.concatenate([oracle.validate_motions(e, s, g)[0] for e, s, g in graze_cases(oracle, lambda _: eps)])
        oks.append(ok.mean())
    print("grazing: oracle valid fractions per epsilon", np.round(oks, 3), flush=True)
    assert oks[0] < oks[-1] and 0.0 < oks[-1] and oks[0] < 1.0


@pytest.mark.gpu
@pytest.mark.parametrize("eps", EPS)
def test_grazing_at_the_clear_threshold(vamp, oracle, eps):
    def eps_of(probe):
        if eps[0] in "+-0":
            return float(eps)
        hdr, _ = gpu_env_from_oracle(vamp, probe()).clear_grid()
        assert hdr is not None
        return float(hdr["margin"]) * float(eps.split("*")[1]) if "margin" in eps else float(np.linalg.norm(hdr["h"]))
    n_ok = n_all = 0
    for oenv, s, g in graze_cases(oracle, eps_of):
        ok, ne = vamp.panda_0_0.validate_batch(s, g, gpu_env_from_oracle(vamp, oenv))
        rok, rne = oracle.validate_motions(oenv, s, g)
        assert np.array_equal(ne, rne) and np.array_equal(ok, rok), eps
        n_ok += int(rok.sum())
        n_all += len(rok)
    print(f"grazing eps {eps}: {n_ok}/{n_all} edges valid", flush=True)


# ---- 4. environments without a grid ------------------------------------------------------------------------------
def no_grid_scenes(oracle):
    rng = np.random.default_rng(21)
    sheared = oracle.sphere_cage_env()
    A = np.eye(3) + rng.uniform(-0.35, 0.35, (3, 3))
    sheared.add_cuboid_axes([0.4, 0.1, 0.5], A[0].astype(F), A[1].astype(F), A[2].astype(F), [0.05, 0.08, 0.04])
    many = oracle.Env()
    for _ in range(CAP + 1):
        many.add_sphere(rng.uniform([-0.8, -0.8, 0.0], [0.8, 0.8, 1.2]).astype(F), F(rng.uniform(0.005, 0.02)))
    nan = oracle.sphere_cage_env()  # a z-cuboid (a3.z == 1) whose test never reads a3.x: the record holds a NaN
    nan.add_cuboid_axes([0.45, -0.2, 0.5], np.array([1, 0, 0], F), np.array([0, 1, 0], F),
                        np.array([np.nan, 0, 1], F), [0.05, 0.05, 0.05])
    assert len(nan.zcuboids) == 1
    return {"sheared_cuboid": sheared, "cap_plus_one": many, "nan_coordinate": nan, "empty": oracle.Env()}


@pytest.mark.gpu
@pytest.mark.parametrize("name", ["sheared_cuboid", "heightfield", "cap_plus_one", "nan_coordinate", "empty"])
def test_no_grid_still_equals_the_oracle(vamp, oracle, name):
    s, g = edges(oracle, 1024, 5)
    if name == "heightfield":
        from scenes import terrain
        hf = terrain()
        hf = ((0.0, 0.0, -0.4), hf[1], hf[2], hf[3])
        oenv = oracle.sphere_cage_env()
        env = gpu_env_from_oracle(vamp, oenv)
        env.add_heightfield(vamp.make_heightfield(*hf))
        oenv.add_heightfield(hf[0], hf[1], hf[2][0], hf[2][1], hf[3])
    else:
        oenv = no_grid_scenes(oracle)[name]
        env = gpu_env_from_oracle(vamp, oenv)
    assert env.clear_grid() == (None, None), f"{name}: this environment must not get a clearance grid"
    ok, ne = vamp.panda_0_0.validate_batch(s, g, env)
    rok, rne = oracle.validate_motions(oenv, s, g)
    assert np.array_equal(ne, rne) and np.array_equal(ok, rok), name
    if name == "cap_plus_one":  # one record fewer: the grid is back, same parity
        oenv.spheres.pop()
        env = gpu_env_from_oracle(vamp, oenv)
        assert env.clear_grid()[0] is not None
        ok, ne = vamp.panda_0_0.validate_batch(s, g, env)
        rok, rne = oracle.validate_motions(oenv, s, g)
        assert np.array_equal(ne, rne) and np.array_equal(ok, rok), "at the cap"


# ---- 5. a grid never outlives its records -----------------------------------------------------------------------
@pytest.mark.gpu
def test_grid_follows_the_environment(vamp, oracle):
    oenv = oracle.sphere_cage_env()
    env = gpu_env_from_oracle(vamp, oenv)
    s, g = edges(oracle, 2048, 9)
    ok, ne = vamp.panda_0_0.validate_batch(s, g, env)
    rok, rne = oracle.validate_motions(oenv, s, g)
    assert np.array_equal(ne, rne) and np.array_equal(ok, rok)
    _, before = env.clear_grid()
    # a sphere across an edge the first call found valid
    e = int(np.flatnonzero(rok & (rne > 1))[0])
    mid = ((s[e].astype(np.float64) + g[e]) / 2).astype(F)
    c = oracle.sphere_fk(mid[None])[0, 40].astype(F)
    oenv.add_sphere(c, F(0.06))
    env.add_sphere(vamp.Sphere(c, 0.06))
    ok2, ne2 = vamp.panda_0_0.validate_batch(s, g, env)
    rok2, rne2 = oracle.validate_motions(oenv, s, g)
    assert not rok2[e] and rok2.sum() < rok.sum()
    assert np.array_equal(ne2, rne2) and np.array_equal(ok2, rok2), "a stale clearance grid"
    _, after = env.clear_grid()
    assert after.shape != before.shape or (after != before).any()
    st = env.upload_stats()
    assert st["tail"] >= 1, "the obstacle was added in place (the tail-only upload rebuilds the grid too)"
    # a cuboid and a capsule on top (other record types), then an attachment and its removal: the records stay
    a = 0.3
    oenv.add_cuboid_axes([0.5, -0.45, 0.55], np.array([np.cos(a), np.sin(a), 0], F),
                         np.array([-np.sin(a), np.cos(a), 0], F), np.array([0, 0, 1], F), [0.05, 0.05, 0.3])
    oenv.add_capsule_endpoints([-0.5, 0.4, 0.3], [-0.3, 0.5, 0.9], F(0.04))
    env = gpu_env_from_oracle(vamp, oenv)
    att, oatt = vamp.Attachment([0, 0, 0.05], (0.0, 0.0, 0.0, 1.0)), oracle.Attachment([0, 0, 0.05], (0.0, 0.0, 0.0, 1.0))
    att.add_sphere(vamp.Sphere([0, 0, 0], 0.04))
    oatt.add_sphere([0, 0, 0], 0.04)
    env.attach(att)
    ok3, ne3 = vamp.panda_0_0.validate_batch(s, g, env)
    rok3, rne3 = oracle.robot_validate_motions_att("panda", oenv, oatt, s, g)
    assert np.array_equal(ne3, rne3) and np.array_equal(ok3, rok3), "attached"
    env.detach()
    ok4, ne4 = vamp.panda_0_0.validate_batch(s, g, env)
    rok4, rne4 = oracle.validate_motions(oenv, s, g)
    assert np.array_equal(ne4, rne4) and np.array_equal(ok4, rok4), "detached"


# ---- 6. the knob ---------------------------------------------------------------------------------------------------
@pytest.mark.gpu
def test_knob_changes_no_result(tmp_path, oracle):
    res = {}
    for name, val in (("on", None), ("off", "0")):
        out = str(tmp_path / f"{name}.npz")
        env = dict(os.environ)
        env.pop("VAMP_AMD_CLEAR", None)
        if val is not None:
            env["VAMP_AMD_CLEAR"] = val
        r = subprocess.run([sys.executable, os.path.join(HERE, "clear_probe.py"), out], env=env, capture_output=True,
                           text=True, timeout=240)
        assert r.returncode == 0, r.stderr[-2000:]
        res[name] = dict(np.load(out, allow_pickle=False))
    assert bool(res["on"]["grid"]) and not bool(res["off"]["grid"])
    assert np.array_equal(res["on"]["ok"], res["off"]["ok"]) and np.array_equal(res["on"]["n"], res["off"]["n"])
    s, g = clear_batch()
    rok, rne = oracle.validate_motions(oracle.sphere_cage_env(), oracle.scale(s), oracle.scale(g))
    assert np.array_equal(res["on"]["ok"], rok) and np.array_equal(res["on"]["n"], rne)
    assert 0 < rok.mean() < 1
