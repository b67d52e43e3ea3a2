"""Neighbour-query cases with caller-chosen k, r and kmax, shared by tests/test_knn_params.py (the CPU k-d
tree), tests/test_gpu_knn_params.py (the GPU kernels) and tests/knn_probe.py (the kernel variants).

Plain numpy, seeded.  A case is (V [n, dim], k [n], r [n], kmax, ranges): k and r are indexed by vertex,
ranges lists the (q_first, q_count) query ranges asked of it.  Case.ref(i) is the plain loop's answer
(oracle_py.roadmap_knn_kr) for range i, computed once and shared; nobody writes to it.

Every generator asserts on the oracle's answer that the case holds what it is for (rows that end empty,
rows that fill up, a candidate exactly on the radius, cut tie groups): these are conditions of the case, not
measurements of the code under test.

    width-d{8,14}-k{kmax}   every list width: k = kmax, r = +inf, so cnt[i] = min(i, kmax)
    kover-d{7,14}           k[i] up to 64 with kmax = 20: a k above kmax counts as kmax
    edges-d{6,8}            admission edges: r = 0, d == r, just below d, +inf, below every distance; k from 0
    ties-d{6,7}             lattice points: equal distances, duplicates, tie groups cut by k
    geom-{clusters,segment,outlier}-d{8,14}   what the index's boxes and Morton keys can get wrong
    size-n{1..4097}         one partial tile, the tile and super-tile boundaries, sub-ranges
    super-d8                more than 64 super-tiles (n = 300000), two query ranges only
"""
import functools

import numpy as np

F = np.float32
INF = F(np.inf)
WIDTHS = (1, 16, 17, 32, 33, 40, 41, 48, 49, 64)
SIZES = (1, 2, 3, 63, 64, 65, 4095, 4096, 4097)
GEOM = ("clusters", "segment", "outlier")


def _oracle():
    import oracle_py
    return oracle_py


class Case:
    def __init__(self, name, V, k, r, kmax, ranges=None):
        self.name = name
        self.V = np.ascontiguousarray(V, F)
        self.n, self.dim = self.V.shape
        self.k = np.ascontiguousarray(k, np.uint32)
        self.r = np.ascontiguousarray(r, F)
        self.kmax = int(kmax)
        self.ranges = list(ranges) if ranges is not None else [(0, self.n)]
        self._ref = {}
        for a in (self.V, self.k, self.r):
            a.setflags(write=False)

    def ref(self, i=0):
        """(nbr [q_count, kmax], dist, cnt) of range i by the plain loop"""
        if i not in self._ref:
            qf, qc = self.ranges[i]
            out = _oracle().roadmap_knn_kr(self.V, self.k, self.r, self.kmax, np.arange(qf, qf + qc, dtype=np.uint32))
            for a in out:
                a.setflags(write=False)
            self._ref[i] = out
        return self._ref[i]

    def queries(self):
        """every queried vertex, in range order"""
        return np.concatenate([np.arange(qf, qf + qc, dtype=np.uint32) for qf, qc in self.ranges])


def same_lists(got, want, kmax):
    """cnt equal, nbr and dist bit for bit on the first cnt slots; nothing is asked of the slots beyond"""
    gn, gd, gc = got
    wn, wd, wc = want
    gc = np.asarray(gc).view(np.uint32)
    assert np.array_equal(gc, wc), f"cnt differs in {int((gc != wc).sum())} rows, first {np.nonzero(gc != wc)[0][:5]}"
    mask = np.arange(kmax)[None, :] < wc[:, None]
    gn = np.asarray(gn).view(np.uint32)[:len(wc)]
    gd = np.asarray(gd)[:len(wc)].view(np.uint32)
    bad = (gn != wn) & mask
    assert not bad.any(), f"nbr differs in rows {np.nonzero(bad.any(1))[0][:5]}"
    bad = (gd != wd.view(np.uint32)) & mask
    assert not bad.any(), f"dist differs in rows {np.nonzero(bad.any(1))[0][:5]}"


def _nearest(V, kk):
    """the kk nearest earlier vertices of every vertex (r = +inf) by the plain loop"""
    n = len(V)
    return _oracle().roadmap_knn_kr(V, np.full(n, kk, np.uint32), np.full(n, INF, F), kk)


def _tenth(V):
    """median distance to the 10th nearest earlier vertex at the set's final density: over the last twentieth
    of the rows, whose prefixes hold nearly every vertex (the early rows' sparse prefixes would only enlarge it)"""
    _, d, c = _nearest(V, 10)
    lo = len(V) - len(V) // 20
    return F(np.median(d[lo:][c[lo:] == 10, 9]))


def _fraction(x):
    return float(np.mean(x))


# ---- case 1: every list width --------------------------------------------------------------------------------
def width(dim, kmax):
    n = 600
    rng = np.random.default_rng(100 + dim)
    V = rng.random((n, dim), dtype=F)
    c = Case(f"width-d{dim}-k{kmax}", V, np.full(n, kmax, np.uint32), np.full(n, INF, F), kmax)
    cnt = c.ref()[2]
    assert cnt[0] == cnt[1] == 0 and np.array_equal(cnt[2:], np.minimum(np.arange(2, n), kmax))
    return c


# ---- case 2: k above kmax ------------------------------------------------------------------------------------
def kover(dim):
    n, kmax = 600, 20
    rng = np.random.default_rng(200 + dim)
    V = rng.random((n, dim), dtype=F)
    k = rng.integers(0, 65, n).astype(np.uint32)
    r = np.where(rng.random(n) < 0.5, INF, _tenth(V)).astype(F)
    assert (k > kmax).sum() >= 100
    c = Case(f"kover-d{dim}", V, k, r, kmax)
    cnt = c.ref()[2]
    assert cnt.max() == kmax and ((cnt == kmax) & (k > kmax)).sum() >= 100
    return c


# ---- case 3: admission edges ---------------------------------------------------------------------------------
def edges(dim):
    n, kmax = 1500, 24
    rng = np.random.default_rng(300 + dim)
    V = rng.random((n, dim), dtype=F)
    form = np.arange(n) % 6
    b = rng.choice(np.arange(200, n), 30, replace=False)  # 30 exact duplicate pairs (a < b)
    a = (rng.random(30) * (b - 2)).astype(np.int64) + 2
    a = np.where(np.isin(a, b), 2, a)  # a vertex is not both copy and original (2 is below every b)
    V[b] = V[a]
    form[b[:15]] = 0  # r = 0 with a duplicate at distance 0 in half of the pairs
    k = rng.integers(0, kmax + 1, n).astype(np.uint32)
    nn, nd, nc = _nearest(V, 12)
    r = np.zeros(n, F)
    star = np.full(n, -1, np.int64)
    for i in range(2, n):
        f = form[i]
        if f == 1:  # a small quantile of the row's distances
            r[i] = F(np.quantile(np.linalg.norm(V[:i].astype(np.float64) - V[i], axis=1), 0.02))
        elif f in (2, 3):  # the oracle's float distance to one of the 12 nearest, or the float just below it
            m = int(rng.integers(0, nc[i]))
            star[i] = nn[i, m]
            r[i] = nd[i, m] if f == 2 else np.nextafter(nd[i, m], F(0))
        elif f == 4:
            r[i] = INF
        elif f == 5:  # below every distance
            r[i] = nd[i, 0] * F(0.5) if nd[i, 0] > 0 else F(-1)
    c = Case(f"edges-d{dim}", V, k, r, kmax)
    onb, od, oc = c.ref()
    kk = np.minimum(k, kmax)
    rows = np.arange(n) >= 2
    assert _fraction(oc[rows] == 0) >= 0.05
    assert _fraction((oc[rows] == kk[rows]) & (kk[rows] > 0)) >= 0.20
    last = np.zeros(n, bool)
    for i in np.nonzero((form == 2) & rows & (oc > 0))[0]:
        last[i] = od[i, oc[i] - 1] == r[i] and onb[i, oc[i] - 1] == star[i]
    assert last.sum() >= 50, int(last.sum())
    assert ((form == 0) & (oc > 0)).sum() >= 10  # r = 0 finds the duplicates
    return c


# ---- case 4: ties --------------------------------------------------------------------------------------------
def ties(dim):
    n, kmax = 2000, 16
    rng = np.random.default_rng(400 + dim)
    V = (rng.integers(0, 3, (n, dim)) * 0.25).astype(F)  # exact in float32
    k = rng.choice(np.array([1, 5, 16], np.uint32), n)
    r = rng.choice(np.array([0.25, 0.5, np.inf], F), n)
    c = Case(f"ties-d{dim}", V, k, r, kmax)
    # rows whose k-th and (k+1)-th candidates are equally far: the same query with one more slot
    _, d1, c1 = _oracle().roadmap_knn_kr(V, k + 1, r, kmax + 1)
    ki = k.astype(np.int64)
    cut = (c1 > ki) & (d1[np.arange(n), ki - 1] == d1[np.arange(n), np.minimum(ki, kmax)])
    assert cut.sum() >= 200, int(cut.sum())
    return c


# ---- case 5: index geometry ----------------------------------------------------------------------------------
def geom(kind, dim):
    n, kmax = 5000, 24
    rng = np.random.default_rng(800 + dim + 20 * GEOM.index(kind))  # seeds at which the conditions below hold
    if kind == "clusters":  # 20 Gaussian clusters of sigma 1e-3 and 5 % uniform background
        centre = rng.random((20, dim))
        V = centre[rng.integers(0, 20, n)] + rng.normal(0, 1e-3, (n, dim))
        bg = rng.random(n) < 0.05
        V[bg] = rng.random((int(bg.sum()), dim))
    elif kind == "segment":  # every coordinate but one is constant
        V = np.tile(rng.random(dim), (n, 1))
        V[:, dim // 2] = rng.random(n)
    else:  # a uniform cloud and one far outlier, early enough to lie in most prefixes
        V = rng.random((n, dim))
        V[10] = 1e6
    V = V.astype(F)
    r = np.where(rng.random(n) < 0.5, INF, _tenth(V)).astype(F)
    c = Case(f"geom-{kind}-d{dim}", V, np.full(n, kmax, np.uint32), r, kmax)
    cnt = c.ref()[2][2:]
    assert _fraction(cnt == 0) >= 0.05 and _fraction(cnt == 24) >= 0.20, (_fraction(cnt == 0), _fraction(cnt == 24))
    return c


# ---- case 6: structural sizes --------------------------------------------------------------------------------
def size(n):
    rng = np.random.default_rng(600 + n)
    V = rng.random((n, 8), dtype=F)
    ranges = [(0, n), (0, 1)]
    if n >= 6:
        ranges.append((1, 5))
    if n >= 3:
        ranges.append((n - 3, 3))
    return Case(f"size-n{n}", V, np.full(n, 16, np.uint32), np.full(n, INF, F), 16, ranges)


# ---- case 7: more than 64 super-tiles ------------------------------------------------------------------------
def _halton(n, dim):
    """Halton points 1 .. n in the unit cube (radical inverses in the first primes)"""
    out = np.zeros((n, dim))
    for d, p in enumerate((2, 3, 5, 7, 11, 13, 17, 19)[:dim]):
        i = np.arange(1, n + 1, dtype=np.int64)
        f = 1.0
        while i.any():
            f /= p
            out[:, d] += f * (i % p)
            i //= p
    return out.astype(F)


def super_tiles():
    n, dim, kmax = 300000, 8, 48
    assert n > 64 * 64 * 64
    rng = np.random.default_rng(700)
    V = _halton(n, dim)
    V[100000:105000] = (rng.random(dim) + rng.normal(0, 1e-3, (5000, dim))).astype(F)
    o = _oracle()
    r = np.full(n, INF, F)
    ranges = [(131000, 512), (n - 512, 512)]
    for qf, qc in ranges:
        for i in range(qf + 1 - qf % 2, qf + qc, 2):  # odd rows: the PRM* radius of the unit cube
            r[i] = o.prm_neighbor_radius(dim, 1.0, 2.0, i)
    return Case("super-d8", V, np.full(n, kmax, np.uint32), r, kmax, ranges)


# ---- registry ------------------------------------------------------------------------------------------------
BUILDERS = {}
for _d in (8, 14):
    for _k in WIDTHS:
        BUILDERS[f"width-d{_d}-k{_k}"] = functools.partial(width, _d, _k)
for _d in (7, 14):
    BUILDERS[f"kover-d{_d}"] = functools.partial(kover, _d)
for _d in (6, 8):
    BUILDERS[f"edges-d{_d}"] = functools.partial(edges, _d)
for _d in (6, 7):
    BUILDERS[f"ties-d{_d}"] = functools.partial(ties, _d)
for _d in (8, 14):
    for _g in GEOM:
        BUILDERS[f"geom-{_g}-d{_d}"] = functools.partial(geom, _g, _d)
for _n in SIZES:
    BUILDERS[f"size-n{_n}"] = functools.partial(size, _n)
SMALL = list(BUILDERS)  # cases 1-6
BUILDERS["super-d8"] = super_tiles
# what the kernel variants run (tests/knn_probe.py): cases 1 (three widths), 2, 4, 5 and 6
PROBE = [c for c in SMALL if c.split("-")[0] in ("kover", "ties", "geom", "size")
         or (c.startswith("width") and c.rsplit("-k", 1)[1] in ("16", "33", "64"))]


@functools.lru_cache(maxsize=None)
def get(name):
    return BUILDERS[name]()
