"""vamp_amd -- MI355X (gfx950) implementation of VAMP's motion-validation rake.

Host-side mirror of the reference's Python surface for this path
(``vamp.Environment``/``Sphere``/``Cuboid``/``Cylinder`` and ``vamp.<robot>.fk``/``validate``;
reference src/impl/vamp/bindings/environment.cc:18-146 and bindings/common.hh:132-182,586-725),
plus the batch entry points the GPU path exists for.  Every call goes through the C ABI
(include/vamp_gpu.h) into libvampgpu.so; nothing here computes collision results on the CPU.

    import vamp_amd as vamp
    env = vamp.Environment()
    env.add_sphere(vamp.Sphere([0.5, 0.0, 0.3], 0.2))
    vamp.panda.validate(q, env)                      # one configuration (bindings/common.hh:172-190)
    ok, n = vamp.panda_0_0.validate_batch(starts, goals, env)   # N edges, validate_motion each
"""
from __future__ import annotations

import ctypes as C
import weakref
from typing import Dict, List, Optional, Sequence, Tuple

import numpy as np

from . import _lib
from ._lib import VgpuError, check, load

__all__ = [
    "Context", "context", "Environment", "Attachment", "Sphere", "Cuboid", "Cylinder", "HeightField", "make_heightfield", "Robot", "halton", "compact_device",
    "PandaBase", "panda", "panda_0_0", "VgpuError", "SimplifySettings", "SimplifyRoutine", "BSplineSettings",
]


def _f3(v) -> C.Array:
    a = (C.c_float * 3)(*[float(np.float32(x)) for x in v])
    return a


class Context:
    """One HIP device + stream (vgpu_ctx).  Probes the host rsqrt approximation on creation."""

    def __init__(self, device: int = 0):
        lib = load()
        h = C.c_void_p()
        rc = lib.vgpu_ctx_create(int(device), C.byref(h))
        if rc != 0:
            raise VgpuError(f"vgpu_ctx_create(device={device}) failed: {_lib.ERRORS.get(rc, rc)}")
        self.h = h
        self.device = device

    def close(self):
        if getattr(self, "h", None):
            load().vgpu_ctx_destroy(self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def sync(self):
        check(load().vgpu_sync(self.h), self.h)

    def set_stream(self, stream_handle: Optional[int]):
        check(load().vgpu_ctx_set_stream(self.h, C.c_void_p(stream_handle or 0)), self.h)

    def set_profiling(self, enable: bool):
        check(load().vgpu_ctx_set_profiling(self.h, int(bool(enable))), self.h)

    def phase_times(self) -> dict:
        """Accumulated ms of vgpu_validate_motions phases since the last call (then reset)."""
        out = (C.c_float * 4)()
        check(load().vgpu_phase_times(self.h, out), self.h)
        return {"head_ms": out[0], "scan_ms": out[1], "tail_ms": out[2], "calls": int(out[3])}

    def rsqrt_table(self) -> Tuple[np.ndarray, int]:
        k = C.c_int()
        p = _lib.U32P()
        check(load().vgpu_rsqrt_table(self.h, C.byref(k), C.byref(p)), self.h)
        n = 2 << k.value
        return np.ctypeslib.as_array(p, shape=(n,)).copy(), k.value

    def set_rsqrt_table(self, table: np.ndarray, kbits: int):
        t = np.ascontiguousarray(table, np.uint32)
        check(load().vgpu_rsqrt_table_set(self.h, t.ctypes.data_as(_lib.U32P), int(kbits)), self.h)


_contexts: Dict[int, Context] = {}


def context(device: int = 0) -> Context:
    if device not in _contexts:
        _contexts[device] = Context(device)
    return _contexts[device]


# ---- shapes (collision/shapes.hh, factory.hh) ---------------------------------------------
class Sphere:
    """vamp.Sphere(center, radius) (bindings/environment.cc:20-25)."""

    def __init__(self, center: Sequence[float], radius: float):
        self.center = [float(c) for c in center]
        self.r = float(radius)
        self.name = ""

    @property
    def x(self):
        return self.center[0]

    @property
    def y(self):
        return self.center[1]

    @property
    def z(self):
        return self.center[2]

    @property
    def position(self):
        return list(self.center)

    def __repr__(self):
        return f"Sphere({self.center}, {self.r})"


class Cuboid:
    """vamp.Cuboid(center, euler_xyz, half_extents) (bindings/environment.cc:70-76); use
    Cuboid.from_axes for resolved axes (the Euler->axes step of factory.hh:26-60 goes through
    Eigen in the reference and is restated here without bit-parity)."""

    def __init__(self, center, euler_xyz=None, half_extents=None, axes=None):
        self.center = [float(c) for c in center]
        self.euler = None if euler_xyz is None else [float(e) for e in euler_xyz]
        self.half = [float(h) for h in half_extents]
        self.axes = axes
        self.name = ""

    @classmethod
    def from_axes(cls, center, axis_1, axis_2, axis_3, half_extents):
        return cls(center, None, half_extents, axes=[list(axis_1), list(axis_2), list(axis_3)])


class Cylinder:
    """vamp.Cylinder(center, euler_xyz, radius, length) or vamp.Cylinder(endpoint1, endpoint2,
    radius) (bindings/environment.cc:37-52); added to environments as capsules."""

    def __init__(self, a, b, radius, length=None):
        if length is None:
            self.p1, self.p2, self.r = [float(v) for v in a], [float(v) for v in b], float(radius)
            self.center = None
        else:
            self.center, self.euler, self.r, self.length = ([float(v) for v in a], [float(v) for v in b],
                                                            float(radius), float(length))
        self.name = ""


class HeightField:
    """collision::HeightField<float> as made by vamp.make_heightfield(center, scale,
    dimensions, data) (bindings/environment.cc:96-105, factory.hh:365-423): reciprocal scales
    xs/ys/zs = 1/scale, data row-major with dimensions (xd, yd)."""

    def __init__(self, center, scale, dimensions, data):
        self.center = [float(v) for v in center]
        self.scale = [float(v) for v in scale]
        self.xd, self.yd = int(dimensions[0]), int(dimensions[1])
        self.data = np.ascontiguousarray(data, np.float32).ravel()
        if self.data.size != self.xd * self.yd:
            raise ValueError("heightfield data must hold dimensions[0] * dimensions[1] values")
        self.x, self.y, self.z = (np.float32(v) for v in self.center)
        self.xs, self.ys, self.zs = (np.float32(1.0) / np.float32(v) for v in self.scale)


def make_heightfield(center, scale, dimensions, data) -> HeightField:
    return HeightField(center, scale, dimensions, data)


class _PointCloud:
    def __init__(self, points, r_min, r_max, r_point):
        self.points = np.ascontiguousarray(points, np.float32).reshape(-1, 3)
        self.r_min, self.r_max, self.r_point = float(r_min), float(r_max), float(r_point)


class Attachment:
    """collision::Attachment<float> (collision/attachments.hh:14-123; bindings/environment.cc:197-249):
    spheres rigidly attached at a frame relative to the end effector."""

    def __init__(self, center: Sequence[float], quaternion_xyzw: Sequence[float]):
        self.tf = np.array(list(center) + list(quaternion_xyzw), np.float32)
        if self.tf.shape != (7,):
            raise ValueError("center[3] and quaternion_xyzw[4]")
        self.spheres: List[Sphere] = []
        self.posed_spheres: List[Sphere] = []

    @property
    def relative_frame(self):
        return (self.tf[:3].tolist(), self.tf[3:].tolist())

    def add_sphere(self, sphere: Sphere):
        self.spheres.append(sphere)

    def add_spheres(self, spheres: Sequence[Sphere]):
        self.spheres.extend(spheres)

    def set_ee_pose(self, position: Sequence[float], quaternion_xyzw: Sequence[float]):
        """Attachment::pose (attachments.hh:75-122) on the host, float32 left to right (the
        kernels' att_pose / att_sphere): fills posed_spheres."""
        F = np.float32
        ptx, pty, ptz = (F(v) for v in position)
        prx, pry, prz, prw = (F(v) for v in quaternion_xyzw)
        ttx, tty, ttz, trx, try_, trz, trw = (F(v) for v in self.tf)
        two, one = F(2.0), F(1.0)
        with np.errstate(all="ignore"):
            rx = prw * trx + prx * trw + pry * trz - prz * try_
            ry = prw * try_ - prx * trz + pry * trw + prz * trx
            rz = prw * trz + prx * try_ - pry * trx + prz * trw
            rw = prw * trw - prx * trx - pry * try_ - prz * trz
            x0, x1, x2 = pry * ttz - prz * tty, prx * tty - pry * ttx, prx * ttz - prz * ttx
            tx = ptx + two * (prw * x0 + pry * x1 + prz * x2) + ttx
            ty = pty + two * (-prw * x2 - prx * x1 + prz * x0) + tty
            tz = ptz + two * (prw * x1 - prx * x2 - pry * x0) + ttz
            b0, b1, b2, b3, b4 = ry * ry, rz * rz, rw * rz, rw * ry, rx * rx
            b5, b6, b7, b8 = rw * rx, rx * ry, rx * rz, ry * rz
            xx, xy, xz = -two * (b0 + b1) + one, two * (b6 + b2), two * (b7 - b3)
            yx, yy, yz = two * (b6 - b2), -two * (b1 + b4) + one, two * (b8 + b5)
            zx, zy, zz = two * (b7 + b3), two * (b8 - b5), -two * (b0 + b4) + one
            self.posed_spheres = []
            for s in self.spheres:
                x, y, z = (F(v) for v in s.center)
                self.posed_spheres.append(Sphere((x * xx + y * yx + z * zx + tx, x * xy + y * yy + z * zy + ty,
                                                  x * xz + y * yz + z * zz + tz), s.r))

    def _rows(self) -> np.ndarray:
        return np.array([list(s.center) + [s.r] for s in self.spheres], np.float32).reshape(-1, 4)


_ENVS = weakref.WeakSet()  # live environments (the debug build's bounds-check fixture reads their copies)


class Environment:
    """collision::Environment<float> (environment.hh:12-82) realised lazily per Context."""

    def __init__(self):
        _ENVS.add(self)
        self._ops: List[Tuple[str, object]] = []
        self._handles: Dict[int, C.c_void_p] = {}
        self._host: Optional[C.c_void_p] = None  # host-only twin holding the built CAPTs
        self._n_clouds = 0  # point clouds in the twin (built once; realised by copying their arrays)

    def _changed(self):
        """Drop every realised copy (the next use re-creates it from the op list)."""
        for dev, h in list(self._handles.items()):
            load().vgpu_env_destroy(h)
        self._handles.clear()

    def _apply_live(self, op):
        """Apply one op to every realised copy in place: the library re-sends only the section it touches
        (vgpu_env_upload: obstacles / attachment in the blob's tail; the point clouds and their cell grids
        stay on the device unless a cloud is added)."""
        lib = load()
        for key, h in list(self._handles.items()):
            self._apply(lib, h, None, op)

    def _push(self, op):
        """Apply op to every realised copy, then record it.  If it fails on some copy (an invalid shape),
        every copy is dropped and the op is not recorded: the copies cannot diverge, and later contexts
        realise the environment without it."""
        try:
            self._apply_live(op)
        except Exception:
            self._changed()
            raise
        self._ops.append(op)

    def add_sphere(self, s: Sphere):
        self._push(("sphere", s))

    def add_cuboid(self, c: Cuboid):
        self._push(("cuboid", c))

    def add_capsule(self, c: Cylinder):
        self._push(("capsule", c))

    def add_heightfield(self, h: HeightField):
        self._push(("heightfield", h))

    def attach(self, a: Attachment):
        """Environment.attach (bindings/environment.cc:161-162): validate_motion then checks its
        first rake block through Robot::fkcc_attach (planning/validate.hh:43)."""
        self._ops = [op for op in self._ops if op[0] != "attach"]
        self._push(("attach", (a.tf.copy(), a._rows())))

    def detach(self):
        """Environment.detach (bindings/environment.cc:163)."""
        self._ops = [op for op in self._ops if op[0] != "attach"]
        self._apply_live(("detach", None))

    def upload_stats(self, ctx: Optional["Context"] = None) -> dict:
        """vgpu_env_upload_stats of the copy on ctx: whole-blob uploads, tail-only uploads, cell-grid builds."""
        ctx = ctx or context()
        out = (C.c_uint64 * 3)()
        check(load().vgpu_env_upload_stats(self.handle(ctx), out), ctx.h)
        return {"full": int(out[0]), "tail": int(out[1]), "grids": int(out[2])}

    def clear_grid(self, ctx: Optional["Context"] = None):
        """vgpu_env_clear_grid of the copy on ctx: (header dict, cells) with cells a uint8 array indexed
        [iz, iy, ix], or (None, None) when the environment has no clearance grid."""
        ctx = ctx or context()
        hdr = (C.c_float * 18)()
        n = C.c_int32()
        check(load().vgpu_env_clear_grid(self.handle(ctx), hdr, C.byref(n), None, 0), ctx.h)
        if n.value == 0:
            return None, None
        N = int(n.value)
        raw = np.empty(N * N * N, np.uint8)
        check(load().vgpu_env_clear_grid(self.handle(ctx), hdr, C.byref(n), raw.ctypes.data, raw.size), ctx.h)
        h = np.array(hdr[:], np.float32)
        # storage order: bricks (bz, by, bx) of cells (z, y, x)
        B = N // 4
        cells = raw.reshape(B, B, B, 4, 4, 4).transpose(0, 3, 1, 4, 2, 5).reshape(N, N, N)
        return {"lo": h[0:3], "h": h[3:6], "inv_h": h[6:9], "a_lo": h[9:12], "a_hi": h[12:15], "margin": h[15],
                "slack": h[16], "step": h[17], "n": N}, cells

    @property
    def attached(self) -> bool:
        return any(op[0] == "attach" for op in self._ops)

    def _host_env(self):
        if self._host is None:
            h = C.c_void_p()
            check(load().vgpu_env_create(None, C.byref(h)))
            self._host = h
        return self._host

    def add_pointcloud(self, points, r_min: float, r_max: float, r_point: float) -> int:
        """Environment::add_pointcloud (bindings/environment.cc:148-158): builds a CAPT once (host
        twin) and returns the build time in nanoseconds; device environments copy its arrays."""
        pc = _PointCloud(points, r_min, r_max, r_point)
        host = self._host_env()
        ns = C.c_int64()
        check(load().vgpu_env_add_pointcloud(host, pc.points.ctypes.data_as(_lib.F32P), pc.points.shape[0],
                                             pc.r_min, pc.r_max, pc.r_point, C.byref(ns)))
        self._n_clouds += 1
        self._push(("pointcloud", self._n_clouds - 1))
        return int(ns.value)

    def add_pointcloud_device(self, points_ptr: int, n: int, r_min: float, r_max: float, r_point: float,
                              ctx: Optional[Context] = None) -> int:
        """Environment::add_pointcloud with the CAPT built on the GPU (vgpu_capt_build.hip) from
        DEVICE points (n x 3 float32, e.g. a filtered cloud already in HBM); the same arrays as
        add_pointcloud.  The built arrays are kept in the host twin, so the points need not stay
        alive and every context's environment copies them (no rebuild).  Returns the build time in ns."""
        ctx = ctx or context()
        host = self._host_env()
        ns = C.c_int64()
        args = (C.c_void_p(int(points_ptr)), int(n), float(r_min), float(r_max), float(r_point))
        check(load().vgpu_env_add_pointcloud_device(ctx.h, host, *args, C.byref(ns)), ctx.h)
        self._n_clouds += 1
        self._push(("pointcloud", self._n_clouds - 1))
        return int(ns.value)

    def pointcloud_arrays(self, index: int = 0) -> dict:
        """The built CAPT's arrays (tests, aabbs, aff_starts, affordances [n][3][8], top box)."""
        lib = load()
        n2, na, top = C.c_int32(), C.c_size_t(), (C.c_float * 6)()
        check(lib.vgpu_env_pointcloud_info(self._host, index, C.byref(n2), C.byref(na), top))
        m = 1 << n2.value
        tests = np.zeros(max(m - 1, 0), np.float32)
        aabbs = np.zeros((m, 6), np.float32)
        starts = np.zeros(m + 1, np.uint32)
        aff = np.zeros((na.value, 3, 8), np.float32)
        check(lib.vgpu_env_pointcloud_arrays(self._host, index, tests.ctypes.data_as(_lib.F32P),
                                             aabbs.ctypes.data_as(_lib.F32P), starts.ctypes.data_as(_lib.U32P),
                                             aff.ctypes.data_as(_lib.F32P)))
        return {"nlog2": n2.value, "tests": tests, "aabbs": aabbs, "aff_starts": starts, "aff": aff,
                "aabb_top": np.array(top[:], np.float32)}

    def pointcloud_collides(self, centers, radii, index: int = 0, simd: bool = False,
                            ctx: Optional[Context] = None) -> np.ndarray:
        """Raw sphere queries on the GPU: CAPT::collides (capt.hh:403-443), or with simd=True
        one lane of CAPT::collides_simd (capt.hh:457-541)."""
        ctx = ctx or context()
        c = np.ascontiguousarray(centers, np.float32).reshape(-1, 3)
        r = np.ascontiguousarray(radii, np.float32).ravel()
        if r.shape[0] != c.shape[0]:
            raise ValueError("one radius per centre")
        out = np.zeros(c.shape[0], np.uint8)
        check(load().vgpu_pointcloud_collides_host(ctx.h, self.handle(ctx), index, c.ctypes.data_as(_lib.F32P),
                                                   r.ctypes.data_as(_lib.F32P), c.shape[0], int(simd),
                                                   out.ctypes.data_as(_lib.U8P)), ctx.h)
        return out.astype(bool)

    def pointcloud_collides_device(self, centers_ptr: int, radii_ptr: int, n: int, out_ptr: int, index: int = 0,
                                   simd: bool = False, ctx: Optional[Context] = None):
        ctx = ctx or context()
        check(load().vgpu_pointcloud_collides(ctx.h, self.handle(ctx), index, centers_ptr, radii_ptr, n, int(simd),
                                              out_ptr), ctx.h)

    def handle(self, ctx: Context) -> C.c_void_p:
        """This environment realised on ctx (one device copy per context, rebuilt after a change)."""
        key = ctx.h.value  # per context: two contexts may share a device
        if key in self._handles:
            return self._handles[key]
        lib = load()
        h = C.c_void_p()
        check(lib.vgpu_env_create(ctx.h, C.byref(h)), ctx.h)
        self._realise(lib, h, ctx.h)
        check(lib.vgpu_env_upload(h), ctx.h)
        self._handles[key] = h
        return h

    def host_handle(self) -> C.c_void_p:
        """A host-only twin (no context) for the CPU rake (vgpu_cpu_*)."""
        if "cpu" in self._handles:
            return self._handles["cpu"]
        lib = load()
        h = C.c_void_p()
        check(lib.vgpu_env_create(None, C.byref(h)))
        self._realise(lib, h, None)
        self._handles["cpu"] = h
        return h

    def _realise(self, lib, h, ctx_h):
        for op in self._ops:
            self._apply(lib, h, ctx_h, op)

    def _apply(self, lib, h, ctx_h, op):
        kind, s = op
        if kind == "detach":
            rc = lib.vgpu_env_detach(h)
        elif kind == "sphere":
            rc = lib.vgpu_env_add_sphere(h, _f3(s.center), float(np.float32(s.r)))
        elif kind == "cuboid":
            if s.axes is not None:
                rc = lib.vgpu_env_add_cuboid_axes(h, _f3(s.center), _f3(s.axes[0]), _f3(s.axes[1]),
                                                  _f3(s.axes[2]), _f3(s.half))
            else:
                rc = lib.vgpu_env_add_cuboid_euler(h, _f3(s.center), _f3(s.euler), _f3(s.half))
        elif kind == "heightfield":
            rc = lib.vgpu_env_add_heightfield(h, _f3(s.center), _f3(s.scale), s.xd, s.yd,
                                              s.data.ctypes.data_as(_lib.F32P))
        elif kind == "attach":
            tf, rows = s
            rows = np.ascontiguousarray(rows, np.float32)
            rc = lib.vgpu_env_attach(h, tf.ctypes.data_as(_lib.F32P), rows.ctypes.data_as(_lib.F32P),
                                     rows.shape[0])
        elif kind == "pointcloud":  # s = index of the cloud in the host twin
            rc = lib.vgpu_env_copy_pointcloud(h, self._host, int(s))
        else:
            if s.center is None:
                rc = lib.vgpu_env_add_capsule_endpoints(h, _f3(s.p1), _f3(s.p2), float(np.float32(s.r)))
            else:
                rc = lib.vgpu_env_add_capsule_euler(h, _f3(s.center), _f3(s.euler), float(np.float32(s.r)),
                                                    float(np.float32(s.length)))
        check(rc, ctx_h)

    def counts(self, ctx: Optional[Context] = None) -> List[int]:
        ctx = ctx or context()
        out = (C.c_int32 * 5)()
        check(load().vgpu_env_counts(self.handle(ctx), out), ctx.h)
        return list(out)

    def __del__(self):
        try:
            self._changed()
            if self._host is not None:
                load().vgpu_env_destroy(self._host)
                self._host = None
        except Exception:
            pass


# ---- sampling ---------------------------------------------------------------------------------
def filter_pointcloud_indices(pc, min_dist: float, max_range: float, origin, workspace_min, workspace_max,
                              cull: bool = True, ctx: Optional[Context] = None) -> np.ndarray:
    """Indices of the points vamp.filter_pointcloud keeps (collision/filter.hh:175-268), in its
    final space-filling-curve order, computed on the GPU (vgpu_filter.hip)."""
    ctx = ctx or context()
    pc = np.ascontiguousarray(pc, np.float32).reshape(-1, 3)
    out = np.zeros(max(pc.shape[0], 1), np.uint32)
    cnt = C.c_size_t(0)
    o, lo, up = (np.ascontiguousarray(v, np.float32).reshape(3) for v in (origin, workspace_min, workspace_max))
    check(load().vgpu_filter_pointcloud_host(ctx.h, pc.ctypes.data_as(_lib.F32P), pc.shape[0], float(min_dist),
                                             float(max_range), o.ctypes.data_as(_lib.F32P),
                                             lo.ctypes.data_as(_lib.F32P), up.ctypes.data_as(_lib.F32P), int(cull),
                                             out.ctypes.data_as(_lib.U32P), C.byref(cnt)), ctx.h)
    return out[:cnt.value].copy()


def filter_pointcloud(pc, min_dist: float, max_range: float, origin, workspace_min, workspace_max,
                      cull: bool = True, ctx: Optional[Context] = None) -> np.ndarray:
    """vamp.filter_pointcloud (bindings/common.hh, collision/filter.hh:175-268): the kept points."""
    pc = np.ascontiguousarray(pc, np.float32).reshape(-1, 3)
    return pc[filter_pointcloud_indices(pc, min_dist, max_range, origin, workspace_min, workspace_max, cull, ctx)]


def halton(dim: int, first: int, n: int, ctx: Optional[Context] = None) -> np.ndarray:
    """rng::Halton<dim>::next draws first .. first+n-1 (1-based) of a fresh sampler, on the GPU."""
    ctx = ctx or context()
    out = np.empty((n, dim), np.float32)
    check(load().vgpu_halton_host(ctx.h, dim, first, n, out.ctypes.data_as(_lib.F32P)), ctx.h)
    return out


def compact_device(rows_ptr: int, valid_ptr: int, n: int, dim: int, rows_out_ptr: int, index_out_ptr: int,
                   ctx: Optional[Context] = None) -> int:
    """Stream compaction on the device (selected row indices ascending); returns the count."""
    ctx = ctx or context()
    cnt = C.c_size_t()
    check(load().vgpu_compact(ctx.h, C.c_void_p(rows_ptr or 0), C.c_void_p(valid_ptr), n, dim,
                              C.c_void_p(rows_out_ptr or 0), C.c_void_p(index_out_ptr), C.byref(cnt)), ctx.h)
    return int(cnt.value)


# ---- planning (RRT-Connect on the CPU rake: BASELINE configs[0]) -------------------------------
class RRTCSettings:
    """vamp::planning::RRTCSettings (planning/rrtc_settings.hh:5-20), same field names/defaults."""

    def __init__(self, **kw):
        self.range = 2.0
        self.dynamic_domain = True
        self.radius = 4.0
        self.alpha = 0.0001
        self.min_radius = 1.0
        self.balance = True
        self.tree_ratio = 1.0
        self.max_iterations = 100000
        self.max_samples = 100000
        self.start_tree_first = True
        for k, v in kw.items():
            if not hasattr(self, k):
                raise AttributeError(k)
            setattr(self, k, v)

    def c(self) -> _lib.VgpuRrtcSettings:
        return _lib.VgpuRrtcSettings(float(self.range), int(self.dynamic_domain), float(self.radius),
                                     float(self.alpha), float(self.min_radius), int(self.balance),
                                     float(self.tree_ratio), int(self.max_iterations), int(self.max_samples),
                                     int(self.start_tree_first))


class SimplifyRoutine:
    """vamp::planning::SimplifyRoutine (planning/simplify_settings.hh:7-13)."""
    BSPLINE, REDUCE, SHORTCUT, PERTURB = 0, 1, 2, 3


class BSplineSettings:
    """vamp::planning::BSplineSettings (planning/simplify_settings.hh:15-20)."""

    def __init__(self):
        self.max_steps = 1
        self.min_change = 0.1
        self.midpoint_interpolation = 0.5


class SimplifySettings:
    """vamp::planning::SimplifySettings (planning/simplify_settings.hh:41-51), same field names and defaults:
    max_iterations, interpolate, operations, bspline.{max_steps, min_change, midpoint_interpolation}.
    SHORTCUT and BSPLINE are built; REDUCE, PERTURB and a non-zero `interpolate` raise (unsupported).
    max_path_len is an extension: a path stops before a subdivide that would exceed it (0 = no limit on the
    CPU, the buffer's capacity in a batch)."""

    def __init__(self, **kw):
        self.max_iterations = 5
        self.interpolate = 0
        self.operations = [SimplifyRoutine.SHORTCUT, SimplifyRoutine.BSPLINE]
        self.bspline = BSplineSettings()
        self.max_path_len = 0
        for k, v in kw.items():
            if not hasattr(self, k):
                raise AttributeError(k)
            setattr(self, k, v)

    def c(self) -> _lib.VgpuSimplifySettings:
        ops = [int(o) for o in self.operations]
        if len(ops) > 8:
            raise ValueError("at most 8 operations")
        return _lib.VgpuSimplifySettings(int(self.max_iterations), int(self.interpolate), len(ops),
                                         (C.c_int32 * 8)(*ops), int(self.bspline.max_steps),
                                         float(self.bspline.min_change), float(self.bspline.midpoint_interpolation),
                                         int(self.max_path_len))

    def unsupported(self) -> Optional[str]:
        """the field this build does not support, or None"""
        if self.interpolate:
            return "interpolate"
        for o in self.operations:
            if int(o) in (SimplifyRoutine.REDUCE, SimplifyRoutine.PERTURB):
                return "operations: " + ("REDUCE" if int(o) == SimplifyRoutine.REDUCE else "PERTURB")
        return None


class Halton:
    """rng::Halton<dim> (random/halton.hh) as the planners consume it: vamp.<robot>.halton() with
    reset() / skip(n) / next(); the state is the 1-based index of the next draw."""

    def __init__(self, dim: int):
        self.dim = dim
        self.index = 1

    def reset(self):
        self.index = 1

    def skip(self, n: int):
        self.index += int(n)


class PRMNeighborParams:
    """vamp.PRMNeighborParams(dim, space_measure) = planning::PRMStarNeighborParams (roadmap.hh:42-77,
    bindings/settings.cc:38-44): PRM* k(n) = ceil((e + e/dim) ln n), r(n) from the space measure,
    gamma_scale 2.0."""

    def __init__(self, dim: int, space_measure: float):
        self.dim = int(dim)
        self.space_measure = float(space_measure)
        self.gamma_scale = 2.0

    def _kr(self, num_states: int):
        from .roadmap import prm_neighbor_params
        k, r = prm_neighbor_params(self.dim, self.space_measure, int(num_states) + 1, self.gamma_scale)
        return int(k[num_states]), float(r[num_states])

    def max_neighbors(self, num_states: int) -> int:
        return self._kr(num_states)[0]

    def neighbor_radius(self, num_states: int) -> float:
        return self._kr(num_states)[1]


class PRMSettings:
    """vamp.PRMSettings(neighbor_params) = RoadmapSettings<PRMStarNeighborParams> (roadmap.hh:150-171,
    bindings/settings.cc:46-53): max_iterations = max_samples = 100000 by default."""

    def __init__(self, neighbor_params: PRMNeighborParams):
        self.neighbor_params = neighbor_params
        self.max_iterations = 100000
        self.max_samples = 100000

    def max_neighbors(self, num_states: int) -> int:
        return self.neighbor_params.max_neighbors(num_states)

    def neighbor_radius(self, num_states: int) -> float:
        return self.neighbor_params.neighbor_radius(num_states)


# vgpu_plan_result as a numpy record (the C layout: _lib.VgpuPlanResult)
_PLAN_RESULT_DTYPE = np.dtype({"names": ["solved", "iterations", "nanoseconds", "size", "cost", "path_len"],
                               "formats": ["<i4", "<u8", "<i8", ("<u8", (2,)), "<f4", "<u8"],
                               "offsets": [0, 8, 16, 24, 40, 48], "itemsize": 56})
assert C.sizeof(_lib.VgpuPlanResult) == _PLAN_RESULT_DTYPE.itemsize


class PlanningResult:
    """vamp::planning::PlanningResult (planning/plan.hh): path, cost, iterations, size, nanoseconds."""

    def __init__(self, path, cost, iterations, size, nanoseconds, solved):
        self.path, self.cost, self.iterations = path, cost, iterations
        self.size, self.nanoseconds, self.solved = size, nanoseconds, solved


# ---- robots -----------------------------------------------------------------------------------
# Robot::space_measure of each robot: the reference's generated constant returned as float
# (panda/fk.hh:88-91 "-> float"), values as extracted into model/<robot>.json; the composite is
# two Pandas (product)
_SPACE_MEASURE = {k: float(np.float32(v)) for k, v in {
    _lib.VGPU_ROBOT_PANDA: 878819.1112640093, _lib.VGPU_ROBOT_FETCH: 269832.2635954135,
    _lib.VGPU_ROBOT_UR5: 700852.7173113511, _lib.VGPU_ROBOT_BAXTER: 89641415145.821,
    _lib.VGPU_ROBOT_PANDA_PAIR: 878819.1112640093 ** 2}.items()}


class Robot:
    """Python face of a vamp::robots robot: PandaBase<X100, Y100, Z100>
    (robots/panda_base.hh:15-75) or Fetch (robots/fetch.hh:8-48)."""

    # scale_configuration q * s_m + s_a, descale (q - s_a) * d_m (panda/fk.hh:14-62, fetch/fk.hh:20-97)
    _SCALE = {
        _lib.VGPU_ROBOT_PANDA: (
            [5.9342, 3.6652, 5.9342, 3.2289, 5.9342, 3.9095999999999997, 5.9342],
            [-2.9671, -1.8326, -2.9671, -3.1416, -2.9671, -0.0873, -2.9671],
            [0.1685147113342995, 0.2728364072901888, 0.1685147113342995, 0.30970299482796, 0.1685147113342995,
             0.25578064252097404, 0.1685147113342995]),
        _lib.VGPU_ROBOT_UR5: (
            [6.2831853, 6.2831853, 6.2831853, 6.2831853, 6.2831853, 6.2831853],
            [-3.14159265, -3.14159265, -3.14159265, -3.14159265, -3.14159265, -3.14159265],
            [0.15915494327375637, 0.15915494327375637, 0.15915494327375637, 0.15915494327375637, 0.15915494327375637, 0.15915494327375637]),
        _lib.VGPU_ROBOT_BAXTER: (
            [3.40335987756, 3.194, 6.10835987756, 2.6679999999999997, 6.118, 3.66479632679, 6.118, 3.40335987756, 3.194, 6.10835987756, 2.6679999999999997, 6.118, 3.66479632679, 6.118],
            [-1.70167993878, -2.147, -3.05417993878, -0.05, -3.059, -1.57079632679, -3.059, -1.70167993878, -2.147, -3.05417993878, -0.05, -3.059, -1.57079632679, -3.059],
            [0.2938272871445316, 0.31308703819661865, 0.16371006621166082, 0.37481259370314846, 0.16345210853220005, 0.2728664599148137, 0.16345210853220005, 0.2938272871445316, 0.31308703819661865, 0.16371006621166082, 0.37481259370314846, 0.16345210853220005, 0.2728664599148137, 0.16345210853220005]),
        _lib.VGPU_ROBOT_FETCH: (
            [0.38615, 3.2112, 2.739, 6.28318, 4.502, 6.28318, 4.32, 6.28318],
            [0.0, -1.6056, -1.221, -3.14159, -2.251, -3.14159, -2.16, -3.14159],
            [2.589667227761233, 0.31141006477329347, 0.36509675063891933, 0.15915507752443828,
             0.22212350066637052, 0.15915507752443828, 0.23148148148148145, 0.15915507752443828]),
    }

    def __init__(self, name: str, base_x100: int, base_y100: int, base_z100: int, kind: int = _lib.VGPU_ROBOT_PANDA,
                 base2=(0, 0, 0)):
        self.name = name
        self.c_robot = _lib.VgpuRobot(kind, base_x100, base_y100, base_z100, *base2)
        self._info = None
        self.kind = kind
        if kind == _lib.VGPU_ROBOT_PANDA_PAIR:  # both arms' scaling, concatenated
            sm, sa, dm = (a + a for a in self._SCALE[_lib.VGPU_ROBOT_PANDA])
        else:
            sm, sa, dm = self._SCALE[kind]
        self.S_M = np.array(sm, np.float32)
        self.S_A = np.array(sa, np.float32)
        self.D_M = np.array(dm, np.float32)
        self.radii = {_lib.VGPU_ROBOT_PANDA: _PANDA_RADII, _lib.VGPU_ROBOT_FETCH: _FETCH_RADII,
                      _lib.VGPU_ROBOT_UR5: _UR5_RADII, _lib.VGPU_ROBOT_BAXTER: _BAXTER_RADII}.get(
            kind, np.concatenate([_PANDA_RADII, _PANDA_RADII]))

    def _meta(self):
        if self._info is None:
            dim, res, ns = C.c_int32(), C.c_int32(), C.c_int32()
            check(load().vgpu_robot_info(self.kind, C.byref(dim), C.byref(res), C.byref(ns)))
            self._info = (dim.value, res.value, ns.value)
        return self._info

    def dimension(self) -> int:
        return self._meta()[0]

    def resolution(self) -> int:
        return self._meta()[1]

    def space_measure(self) -> float:
        """Robot::space_measure (robots/panda_base.hh:22 -> panda/fk.hh; fetch.hh:14): the product
        of the joint ranges, the PRMNeighborParams input (src/vamp/__init__.py:91)."""
        return _SPACE_MEASURE[self.kind]

    def n_spheres(self) -> int:
        return self._meta()[2]

    @property
    def base(self):
        r = self.c_robot
        return (np.float32(r.base_x100) / np.float32(100), np.float32(r.base_y100) / np.float32(100),
                np.float32(r.base_z100) / np.float32(100))

    # --- scaling (robots/panda/fk.hh:34-62) ---
    def scale_configuration(self, u):
        u = np.asarray(u, np.float32)
        return (u.astype(np.float64) * self.S_M + self.S_A).astype(np.float32)

    def descale_configuration(self, q):
        q = np.asarray(q, np.float32)
        return ((q - self.S_A) * self.D_M).astype(np.float32)

    # --- reference-named single calls: the CPU rake (host AVX2, csrc/cpu/), as the reference's
    # single-edge entry points stay on the CPU (a GPU launch costs far more than one edge) ---
    def fk(self, configuration) -> List[Sphere]:
        """vamp.<robot>.fk(q) (bindings/common.hh:132-152): the collision spheres."""
        q = np.asarray(configuration, np.float32).reshape(self.dimension())
        xyz = self.cpu_sphere_fk_block(np.repeat(q[:, None], 8, axis=1))[:, :, 0].T
        radii = self.radii
        return [Sphere(xyz[s], float(radii[s])) for s in range(xyz.shape[0])]

    def validate(self, configuration, environment: Environment) -> bool:
        """vamp.<robot>.validate(q, env) (bindings/common.hh:172-190): bounds check in the
        descaled unit box, then validate_motion<Robot, rake, 1>(q, q, env) -- one broadcast block,
        through fkcc_attach when the environment has an attachment (validate.hh:43)."""
        q = np.asarray(configuration, np.float32).reshape(self.dimension())
        d = self.descale_configuration(q)
        if not ((d <= 1.0).all() and (d >= 0.0).all()):
            return False
        return self.validate_motion(q, q, environment)

    def filter_from_pointcloud(self, pointcloud, configuration, environment: Environment, point_radius: float,
                               ctx: Optional[Context] = None) -> np.ndarray:
        """vamp.<robot>.filter_from_pointcloud(pointcloud, configuration, environment, point_radius)
        (bindings/common.hh:36-87,713): the points that neither overlap the robot's spheres at
        `configuration` nor collide with the environment, in input order, as float32 [m][3] -- on
        the GPU (sphere_fk + one lane per point, vgpu_filter_robot_pointcloud_host)."""
        ctx = ctx or context()
        pc = np.ascontiguousarray(pointcloud, np.float32).reshape(-1, 3)
        q = np.ascontiguousarray(configuration, np.float32).reshape(self.dimension())
        out = np.empty((max(pc.shape[0], 1), 3), np.float32)
        cnt = C.c_size_t(0)
        check(load().vgpu_filter_robot_pointcloud_host(ctx.h, C.byref(self.c_robot), environment.handle(ctx),
                                                       q.ctypes.data_as(_lib.F32P), pc.ctypes.data_as(_lib.F32P),
                                                       pc.shape[0], float(point_radius), out.ctypes.data_as(_lib.F32P),
                                                       C.byref(cnt)), ctx.h)
        return out[:cnt.value].copy()

    def filter_from_pointcloud_device(self, pc_ptr: int, n: int, configuration, environment: Environment,
                                      point_radius: float, keep_ptr: int, ctx: Optional[Context] = None):
        """Device form: pc[n][3] (device) -> keep[n] (device uint8, 1 = kept), stream-ordered."""
        ctx = ctx or context()
        q = np.ascontiguousarray(configuration, np.float32).reshape(self.dimension())
        check(load().vgpu_filter_robot_pointcloud(ctx.h, C.byref(self.c_robot), environment.handle(ctx),
                                                  q.ctypes.data_as(_lib.F32P), C.c_void_p(pc_ptr), int(n),
                                                  float(point_radius), C.c_void_p(keep_ptr)), ctx.h)

    def validate_motion(self, start, goal, environment: Environment) -> bool:
        """planning::validate_motion<Robot, 8, resolution> (planning/validate.hh:67-75)."""
        s = np.ascontiguousarray(start, np.float32).reshape(self.dimension())
        g = np.ascontiguousarray(goal, np.float32).reshape(self.dimension())
        v = C.c_int()
        check(load().vgpu_cpu_validate_motion(C.byref(self.c_robot), environment.host_handle(),
                                              s.ctypes.data_as(_lib.F32P), g.ctypes.data_as(_lib.F32P), C.byref(v)))
        return bool(v.value)

    def eefk(self, configuration):
        """vamp.<robot>.eefk(q) (bindings/common.hh:342-352): (position [3], quaternion x y z w [4])."""
        p = self.eefk_batch(np.asarray(configuration, np.float32)[None])[0]
        return p[:3].copy(), p[3:].copy()

    def eefk_batch(self, q) -> np.ndarray:
        """Robot::eefk of each q[n][dim]: [n][7] (x y z, qx qy qz qw), robot frame."""
        q = np.ascontiguousarray(q, np.float32).reshape(-1, self.dimension())
        out = np.empty((q.shape[0], 7), np.float32)
        check(load().vgpu_cpu_eefk(C.byref(self.c_robot), q.ctypes.data_as(_lib.F32P), q.shape[0],
                                   out.ctypes.data_as(_lib.F32P)))
        return out

    def halton(self) -> Halton:
        """vamp.<robot>.halton(): a fresh Halton<dimension> sampler."""
        return Halton(self.dimension())

    def rrtc(self, start, goals, environment: Environment, settings: Optional[RRTCSettings] = None,
             rng: Optional[Halton] = None) -> PlanningResult:
        """vamp.<robot>.rrtc(start, goal(s), env, settings, rng) (bindings/common.hh:191-200 ->
        planning/rrtc.hh:33-248) on the CPU rake; rng advances by the draws taken."""
        dim = self.dimension()
        s = np.ascontiguousarray(start, np.float32).reshape(dim)
        g = np.ascontiguousarray(goals, np.float32).reshape(-1, dim)
        settings = settings or RRTCSettings()
        rng = rng or self.halton()
        idx = C.c_uint64(rng.index)
        res = _lib.VgpuPlanResult()
        cap = 4096
        while True:
            path = np.empty((cap, dim), np.float32)
            i0 = C.c_uint64(idx.value)
            rc = load().vgpu_cpu_rrtc(C.byref(self.c_robot), environment.host_handle(), s.ctypes.data_as(_lib.F32P),
                                      g.ctypes.data_as(_lib.F32P), g.shape[0], C.byref(settings.c()), C.byref(i0),
                                      path.ctypes.data_as(_lib.F32P), cap, C.byref(res))
            if rc == _lib.VGPU_OK or res.path_len <= cap:
                check(rc)
                idx = i0
                break
            cap = int(res.path_len)
        rng.index = int(idx.value)
        return PlanningResult(path[:res.path_len].copy(), float(res.cost), int(res.iterations),
                              (int(res.size[0]), int(res.size[1])), int(res.nanoseconds), bool(res.solved))

    def simplify(self, path, environment: Environment, settings: Optional[SimplifySettings] = None,
                 rng: Optional[Halton] = None) -> PlanningResult:
        """vamp.<robot>.simplify(path, environment, settings, rng) (bindings/common.hh:677-683 ->
        planning/simplify.hh:192-260) on the CPU rake.  rng is accepted for the reference's signature; the
        supported operations (SHORTCUT, BSPLINE) draw nothing from it.  The result carries `status`
        (0 done, 1 stopped at settings.max_path_len) and `validated_edges` (validate_motion calls made)."""
        dim = self.dimension()
        p = np.ascontiguousarray(path, np.float32).reshape(-1, dim)
        settings = settings or SimplifySettings()
        cs = settings.c()
        res = _lib.VgpuPlanResult()
        st = C.c_int32(0)
        cap = max(4 * p.shape[0], 64)
        while True:
            out = np.empty((cap, dim), np.float32)
            rc = load().vgpu_cpu_simplify(C.byref(self.c_robot), environment.host_handle(),
                                          p.ctypes.data_as(_lib.F32P), p.shape[0], C.byref(cs),
                                          out.ctypes.data_as(_lib.F32P), cap, C.byref(res), C.byref(st))
            if rc == _lib.VGPU_ERR_UNSUPPORTED and settings.unsupported():
                raise VgpuError(f"vamp_gpu: unsupported: simplify: {settings.unsupported()}")
            if rc == _lib.VGPU_OK or res.path_len <= cap:
                check(rc)
                break
            cap = int(res.path_len)
        r = PlanningResult(out[:res.path_len].copy(), float(res.cost), int(res.iterations), [], int(res.nanoseconds),
                           True)
        r.status, r.validated_edges = int(st.value), int(res.size[0])
        return r

    def simplify_capacity(self, max_len: int, settings: SimplifySettings, n_paths: int = 1) -> int:
        """Waypoint slots per path that no simplify run can outgrow: every B-spline step at most doubles the
        segments, (max_len - 1) * 2^(max_iterations * bspline.max_steps) + 1, clamped so that n_paths * capacity
        stays below the batch call's 2^31 limit."""
        steps = int(settings.max_iterations) * int(settings.bspline.max_steps) * sum(
            int(o) == SimplifyRoutine.BSPLINE for o in settings.operations)
        worst = (max(int(max_len), 2) - 1) * 2 ** min(steps, 40) + 1
        return int(max(min(worst, (2 ** 31 - 1) // max(int(n_paths), 1)), 1))

    def simplify_batch(self, paths, environment: Environment, settings: Optional[SimplifySettings] = None,
                       ctx: Optional[Context] = None, capacity: Optional[int] = None):
        """simplify() of every path of a list in one environment, in lockstep on the GPU
        (vgpu_simplify_paths_host): returns ([PlanningResult], status uint8[n]); each result equals
        simplify()'s bit for bit (with settings.max_path_len = capacity where a path stops with status 1).
        capacity: waypoint slots per path, default simplify_capacity() of the longest path."""
        ctx = ctx or context()
        dim = self.dimension()
        settings = settings or SimplifySettings()
        ps = [np.ascontiguousarray(p, np.float32).reshape(-1, dim) for p in paths]
        n = len(ps)
        if n == 0:
            return [], np.zeros(0, np.uint8)
        longest = max(p.shape[0] for p in ps)
        cap = int(capacity) if capacity is not None else self.simplify_capacity(longest, settings, n)
        if cap < longest:
            raise ValueError(f"capacity {cap} below the longest path ({longest} waypoints)")
        w = np.zeros((n, cap, dim), np.float32)
        ln = np.empty(n, np.uint32)
        for i, p in enumerate(ps):
            w[i, :p.shape[0]] = p
            ln[i] = p.shape[0]
        it = np.empty(n, np.uint32)
        st = np.empty(n, np.uint8)
        cost = np.empty(n, np.float32)
        cs = settings.c()
        check(load().vgpu_simplify_paths_host(ctx.h, C.byref(self.c_robot), environment.handle(ctx),
                                              w.ctypes.data_as(_lib.F32P), cap, ln.ctypes.data_as(_lib.U32P), n,
                                              C.byref(cs), it.ctypes.data_as(_lib.U32P), st.ctypes.data_as(_lib.U8P),
                                              cost.ctypes.data_as(_lib.F32P)), ctx.h)
        out = []
        for i in range(n):
            r = PlanningResult(w[i, :ln[i]].copy(), float(cost[i]), int(it[i]), [], 0, True)
            r.status = int(st[i])
            out.append(r)
        return out, st

    def simplify_stats(self, ctx: Optional[Context] = None) -> dict:
        """counters of the context's last simplify_batch / simplify_device call"""
        ctx = ctx or context()
        s = (C.c_uint64 * 3)()
        check(load().vgpu_simplify_stats(ctx.h, s), ctx.h)
        return {"rounds": int(s[0]), "validate_calls": int(s[1]), "edges": int(s[2])}

    # per-problem outcome of rrtc_batch / rrtc_batch_scenes and their device forms (VGPU_RRTC_*)
    RRTC_DONE, RRTC_CAPACITY, RRTC_PATH_CAPACITY = 0, 1, 2

    def rrtc_batch(self, starts, goals, environment: Environment, settings: Optional[RRTCSettings] = None,
                   rng_first=1, node_cap: int = 4096, path_cap: int = 256, ctx: Optional[Context] = None,
                   slice: Optional[int] = None):
        """rrtc() of P start/goal problems in one environment on the GPU, one wave per problem
        (vgpu_rrtc_batch_host): starts [P][dim], goals [P][dim] or [P][n_goals][dim], rng_first the 1-based
        index of each problem's first Halton draw (a scalar, or one per problem).  Returns ([PlanningResult],
        status uint8[P], the advanced indices uint64[P]); each result equals rrtc()'s bit for bit for a sampler
        at rng_first (nanoseconds is 0).  node_cap bounds each problem's trees: the sample limit is
        min(settings.max_samples, node_cap), and a problem that stops there unsolved has status RRTC_CAPACITY.
        A path longer than path_cap has status RRTC_PATH_CAPACITY: its result carries `path_len` and an empty
        path.  slice: iterations per problem and launch (default 256)."""
        ctx = ctx or context()
        dim = self.dimension()
        settings = settings or RRTCSettings()
        s = np.ascontiguousarray(starts, np.float32).reshape(-1, dim)
        n = s.shape[0]
        if n == 0:
            return [], np.zeros(0, np.uint8), np.zeros(0, np.uint64)
        g = np.ascontiguousarray(goals, np.float32).reshape(n, -1, dim)
        idx = np.array(np.broadcast_to(np.asarray(rng_first, np.uint64), (n,)))  # a copy: advanced in place
        node_cap, path_cap = int(node_cap), int(path_cap)
        paths = np.zeros((n, path_cap, dim), np.float32)
        ln = np.zeros(n, np.uint32)
        res = (_lib.VgpuPlanResult * n)()
        st = np.zeros(n, np.uint8)
        cs = settings.c()
        if slice is not None:
            check(load().vgpu_rrtc_set_slice(ctx.h, int(slice)), ctx.h)
        try:
            check(load().vgpu_rrtc_batch_host(ctx.h, C.byref(self.c_robot), environment.handle(ctx),
                                              s.ctypes.data_as(_lib.F32P), g.ctypes.data_as(_lib.F32P), g.shape[1], n,
                                              C.byref(cs), idx.ctypes.data_as(_lib.U64P), node_cap,
                                              paths.ctypes.data_as(_lib.F32P), path_cap, ln.ctypes.data_as(_lib.U32P),
                                              res, st.ctypes.data_as(_lib.U8P)), ctx.h)
        finally:
            if slice is not None:
                load().vgpu_rrtc_set_slice(ctx.h, 0)
        return self._rrtc_results(res, paths, ln, st), st, idx

    def _rrtc_results(self, res, paths, ln, st):
        """[PlanningResult] of a batch's records: one pass over a structured view instead of ctypes field reads
        per problem"""
        rec = np.frombuffer(res, dtype=_PLAN_RESULT_DTYPE)
        solved, its, cost = rec["solved"].tolist(), rec["iterations"].tolist(), rec["cost"].tolist()
        sizes, lens, stl = rec["size"].tolist(), ln.tolist(), st.tolist()
        out = []
        for i in range(len(lens)):
            kept = lens[i] if stl[i] != self.RRTC_PATH_CAPACITY else 0
            pr = PlanningResult(paths[i, :kept].copy(), cost[i], its[i], (sizes[i][0], sizes[i][1]), 0, bool(solved[i]))
            pr.status, pr.path_len = stl[i], lens[i]
            out.append(pr)
        return out

    def rrtc_device(self, starts_ptr: int, goals_ptr: int, n_goals: int, n_problems: int, environment: Environment,
                    settings: Optional[RRTCSettings], rng_index_ptr: int, node_cap: int, paths_ptr: int, path_cap: int,
                    path_len_ptr: int, results_ptr: int, status_ptr: int = 0, ctx: Optional[Context] = None):
        """vgpu_rrtc_batch over device memory: starts float32 [P][dim], goals [P][n_goals][dim], rng_index uint64
        [P] in place, paths float32 [P][path_cap][dim] and path_len uint32 [P] out -- simplify_device's waypoints
        and len --, results [P] vgpu_plan_result records (56 bytes each), status uint8 [P] optional."""
        ctx = ctx or context()
        cs = (settings or RRTCSettings()).c()
        check(load().vgpu_rrtc_batch(ctx.h, C.byref(self.c_robot), environment.handle(ctx), C.c_void_p(starts_ptr),
                                     C.c_void_p(goals_ptr), int(n_goals), int(n_problems), C.byref(cs),
                                     C.c_void_p(rng_index_ptr), int(node_cap), C.c_void_p(paths_ptr), int(path_cap),
                                     C.c_void_p(path_len_ptr), C.c_void_p(results_ptr), C.c_void_p(status_ptr or 0)),
              ctx.h)

    def rrtc_batch_scenes(self, starts, goals, environments: Sequence[Environment], env_index=None,
                          settings: Optional[RRTCSettings] = None, rng_first=1, node_cap: int = 4096,
                          path_cap: int = 256, ctx: Optional[Context] = None, slice: Optional[int] = None):
        """rrtc_batch() with one environment per problem, still one call and one wave per problem
        (vgpu_rrtc_batch_scenes_host): problem p is planned in environments[env_index[p]], and its result equals
        rrtc()'s in that environment bit for bit.  env_index defaults to 0 .. P - 1 when there are as many
        environments as problems and is required otherwise; an environment may be listed twice, shared by several
        problems, or named by none.  Everything else, and the returned triple, is rrtc_batch()'s."""
        dim = self.dimension()
        s = np.ascontiguousarray(starts, np.float32).reshape(-1, dim)
        n = s.shape[0]
        environments = list(environments)
        if env_index is None:
            if len(environments) != n:
                raise ValueError(f"env_index is required: {len(environments)} environments for {n} problems")
            ei = np.arange(n, dtype=np.uint32)
        else:
            ei = np.asarray(env_index)
            if ei.shape != (n,):
                raise ValueError(f"env_index must have one entry per problem ({n}), got shape {ei.shape}")
            if n and (ei.min() < 0 or ei.max() > 0xFFFFFFFF):
                raise ValueError("env_index entries must be unsigned 32-bit indices")
            ei = np.ascontiguousarray(ei, np.uint32)
        ctx = ctx or context()
        settings = settings or RRTCSettings()
        envs = (C.c_void_p * max(len(environments), 1))(*[e.handle(ctx) for e in environments])
        g = np.ascontiguousarray(goals, np.float32).reshape(n, -1, dim) if n else np.zeros((0, 1, dim), np.float32)
        idx = np.array(np.broadcast_to(np.asarray(rng_first, np.uint64), (n,)))  # a copy: advanced in place
        node_cap, path_cap = int(node_cap), int(path_cap)
        paths = np.zeros((n, path_cap, dim), np.float32)
        ln = np.zeros(n, np.uint32)
        res = (_lib.VgpuPlanResult * max(n, 1))()
        st = np.zeros(n, np.uint8)
        cs = settings.c()
        if slice is not None:
            check(load().vgpu_rrtc_set_slice(ctx.h, int(slice)), ctx.h)
        try:
            check(load().vgpu_rrtc_batch_scenes_host(ctx.h, C.byref(self.c_robot), envs, len(environments),
                                                     ei.ctypes.data_as(_lib.U32P), s.ctypes.data_as(_lib.F32P),
                                                     g.ctypes.data_as(_lib.F32P), g.shape[1], n, C.byref(cs),
                                                     idx.ctypes.data_as(_lib.U64P), node_cap,
                                                     paths.ctypes.data_as(_lib.F32P), path_cap,
                                                     ln.ctypes.data_as(_lib.U32P), res, st.ctypes.data_as(_lib.U8P)),
                  ctx.h)
        finally:
            if slice is not None:
                load().vgpu_rrtc_set_slice(ctx.h, 0)
        if n == 0:
            return [], st, idx
        return self._rrtc_results(res, paths, ln, st), st, idx

    def rrtc_scenes_device(self, starts_ptr: int, goals_ptr: int, n_goals: int, n_problems: int,
                           environments: Sequence[Environment], env_index_ptr: int, settings: Optional[RRTCSettings],
                           rng_index_ptr: int, node_cap: int, paths_ptr: int, path_cap: int, path_len_ptr: int,
                           results_ptr: int, status_ptr: int = 0, ctx: Optional[Context] = None):
        """vgpu_rrtc_batch_scenes over device memory: rrtc_device() with environments and env_index uint32 [P] on
        the device (an entry outside the list fails the call).  Problems sorted by scene leave each scene's paths
        a contiguous sub-range of paths / path_len, which simplify_device takes with offset pointers."""
        ctx = ctx or context()
        cs = (settings or RRTCSettings()).c()
        environments = list(environments)
        envs = (C.c_void_p * max(len(environments), 1))(*[e.handle(ctx) for e in environments])
        check(load().vgpu_rrtc_batch_scenes(ctx.h, C.byref(self.c_robot), envs, len(environments),
                                            C.c_void_p(env_index_ptr), C.c_void_p(starts_ptr), C.c_void_p(goals_ptr),
                                            int(n_goals), int(n_problems), C.byref(cs), C.c_void_p(rng_index_ptr),
                                            int(node_cap), C.c_void_p(paths_ptr), int(path_cap),
                                            C.c_void_p(path_len_ptr), C.c_void_p(results_ptr),
                                            C.c_void_p(status_ptr or 0)), ctx.h)

    def rrtc_stats(self, ctx: Optional[Context] = None) -> dict:
        """counters of the context's last rrtc_batch / rrtc_batch_scenes / rrtc_device / rrtc_scenes_device call"""
        ctx = ctx or context()
        s = (C.c_uint64 * 3)()
        check(load().vgpu_rrtc_stats(ctx.h, s), ctx.h)
        return {"launches": int(s[0]), "iterations": int(s[1]), "max_iterations": int(s[2])}

    def roadmap(self, start, goal, environment: Environment, settings: Optional[PRMSettings] = None,
                rng: Optional[Halton] = None, ctx: Optional[Context] = None):
        """vamp.<robot>.roadmap(start, goal, environment, settings, rng) (bindings/common.hh:312-321,667 ->
        PRM::build_roadmap, planning/prm.hh:197-299) on the GPU: the sampler's draws rng.index ..
        rng.index + max_iterations - 1 through the fused Halton -> scale -> fkcc kernel (sharded over
        the ranks when torch.distributed is initialised), the vertex sequence start, goal, valid samples
        in draw order cut at max_samples, then every vertex's PRM* neighbour query and validate_motion
        of its candidates, adjacency in the reference's append order.  Returns a Roadmap with
        vertices, edges, nanoseconds and iterations (= draws taken + 1, the reference loop's count);
        rng advances by the draws taken."""
        import time

        from . import roadmap as _rm
        settings = settings or PRMSettings(PRMNeighborParams(self.dimension(), self.space_measure()))
        rng = rng or self.halton()
        dim = self.dimension()
        s = np.ascontiguousarray(start, np.float32).reshape(dim)
        g = np.ascontiguousarray(goal, np.float32).reshape(dim)
        t0 = time.perf_counter_ns()
        max_it, max_s = int(settings.max_iterations), int(settings.max_samples)
        rows, draws = _rm.roadmap_vertices(self, environment, max_it, rng.index, s, g, max(max_s, 2), ctx)
        draws = draws.cpu().numpy()
        taken = max_it
        if max_s <= 2:  # the loop never draws (nodes.size() < max_samples fails at once)
            taken = 0
        elif len(draws) >= max_s:  # the last vertex's draw ends the loop
            taken = int(draws[max_s - 1]) - rng.index + 1
        rm = _rm.build_roadmap_edges(self, environment, rows.cpu().numpy(),
                                     settings.neighbor_params.gamma_scale, settings.neighbor_params.space_measure,
                                     ctx)
        rng.skip(taken)
        rm.nanoseconds = time.perf_counter_ns() - t0
        rm.iterations = taken + 1
        return rm

    def prm(self, start, goal, environment: Environment, settings: Optional[PRMSettings] = None,
            rng: Optional[Halton] = None, ctx: Optional[Context] = None, _first_chunk: int = 1024) -> PlanningResult:
        """vamp.<robot>.prm(start, goal, environment, settings, rng) (bindings/common.hh:296-310 -> PRM::solve,
        planning/prm.hh:43-196) on the GPU roadmap.  A valid straight line answers at once (path [start, goal],
        iterations 0, size [1, 1], rng untouched).  Otherwise the roadmap is built over a growing number of
        draws (_first_chunk, then x4, clipped by max_iterations and max_samples); the build is causal, so every
        stage's graph is a prefix of the next and the result does not depend on the schedule.  The first stage
        in which start and goal connect gives n* = Roadmap.connect_index(), the vertex at whose insertion the
        reference's union-find joins them; the path is the shortest one over vertices 0 .. n*
        (Roadmap.shortest_paths with limit n*), cost = g[goal], iterations = the draws up to and including
        n*'s, size = [n* + 1, 0], and rng advances by exactly those draws.  Unsolved: empty path, iterations =
        draws taken + 1, size = [vertices, 0].  One goal only: the roadmap fixes start at index 0 and goal at 1."""
        import time

        from . import roadmap as _rm
        dim = self.dimension()
        g = np.ascontiguousarray(goal, np.float32)
        if g.size != dim:
            raise VgpuError("vamp_gpu: unsupported: prm: a list of goals is not supported (one goal configuration)")
        g = g.reshape(dim)
        s = np.ascontiguousarray(start, np.float32).reshape(dim)
        settings = settings or PRMSettings(PRMNeighborParams(dim, self.space_measure()))
        rng = rng or self.halton()
        t0 = time.perf_counter_ns()
        if self.validate_motion(s, g, environment):
            # cost stays 0 as in the reference, which sets it only on the searched branch (plan.hh:175)
            return PlanningResult(np.stack([s, g]), 0.0, 0, [1, 1], time.perf_counter_ns() - t0, True)
        max_it, max_s = int(settings.max_iterations), int(settings.max_samples)
        n_draws = min(max(int(_first_chunk), 1), max_it)
        while True:
            rows, draws = _rm.roadmap_vertices(self, environment, n_draws, rng.index, s, g, max(max_s, 2), ctx)
            draws = draws.cpu().numpy()
            full = max_s <= 2 or len(draws) >= max_s  # the sample limit ends the reference's loop here
            rm = _rm.build_roadmap_edges(self, environment, rows.cpu().numpy(), settings.neighbor_params.gamma_scale,
                                         settings.neighbor_params.space_measure, ctx)
            at = rm.connect_index(0, 1, ctx) if max_s > 2 else None
            if at is not None:
                path, cost, _ = rm.shortest_paths([0], [1], at, ctx)[0]
                taken = int(draws[at]) - rng.index + 1
                rng.skip(taken)
                return PlanningResult(rm.vertices[path.astype(np.int64)].copy(), float(cost), taken, [at + 1, 0],
                                      time.perf_counter_ns() - t0, True)
            if full or n_draws >= max_it:
                taken = 0 if max_s <= 2 else (int(draws[max_s - 1]) - rng.index + 1 if full else max_it)
                rng.skip(taken)
                return PlanningResult(np.zeros((0, dim), np.float32), 0.0, taken + 1, [len(rm.vertices), 0],
                                      time.perf_counter_ns() - t0, False)
            n_draws = min(4 * n_draws, max_it)

    def cpu_validate_vector(self, start, vector, distance: float, environment: Environment) -> bool:
        """planning::validate_vector<Robot, 8, resolution>(start, vector, distance, env)."""
        s = np.ascontiguousarray(start, np.float32).reshape(self.dimension())
        v = np.ascontiguousarray(vector, np.float32).reshape(self.dimension())
        ok = C.c_int()
        check(load().vgpu_cpu_validate_vector(C.byref(self.c_robot), environment.host_handle(),
                                              s.ctypes.data_as(_lib.F32P), v.ctypes.data_as(_lib.F32P),
                                              float(np.float32(distance)), C.byref(ok)))
        return bool(ok.value)

    # --- CPU rake batches and blocks (host numpy in/out; threads <= 0: every hardware thread) ---
    def cpu_fkcc_block(self, block, environment: Environment, attach: bool = False) -> bool:
        """Robot::fkcc<8>(env, block) / fkcc_attach<8>: block = ConfigurationBlock<8> [dim][8]."""
        b = np.ascontiguousarray(block, np.float32).reshape(self.dimension(), 8)
        v = C.c_int()
        fn = load().vgpu_cpu_fkcc_attach_block if attach else load().vgpu_cpu_fkcc_block
        check(fn(C.byref(self.c_robot), environment.host_handle(), b.ctypes.data_as(_lib.F32P), C.byref(v)))
        return bool(v.value)

    def cpu_sphere_fk_block(self, block) -> np.ndarray:
        """Robot::sphere_fk<8>(block): [3][n_spheres][8] world-frame centres."""
        b = np.ascontiguousarray(block, np.float32).reshape(self.dimension(), 8)
        out = np.empty((3, self.n_spheres(), 8), np.float32)
        check(load().vgpu_cpu_sphere_fk_block(C.byref(self.c_robot), b.ctypes.data_as(_lib.F32P),
                                              out.ctypes.data_as(_lib.F32P)))
        return out

    def cpu_fkcc_batch(self, q, environment: Environment, threads: int = 0, attach: bool = False) -> np.ndarray:
        q = np.ascontiguousarray(q, np.float32).reshape(-1, self.dimension())
        out = np.empty(q.shape[0], np.uint8)
        fn = load().vgpu_cpu_fkcc_attach if attach else load().vgpu_cpu_fkcc
        check(fn(C.byref(self.c_robot), environment.host_handle(), q.ctypes.data_as(_lib.F32P), q.shape[0],
                 out.ctypes.data_as(_lib.U8P), int(threads)))
        return out.astype(bool)

    def cpu_validate_mask(self, starts, goals, environment: Environment, threads: int = 0):
        """Full-mask validate on the CPU rake: (ok, n_e, block_ok [sum n_e], block offsets [n+1])."""
        s = np.ascontiguousarray(starts, np.float32).reshape(-1, self.dimension())
        g = np.ascontiguousarray(goals, np.float32).reshape(-1, self.dimension())
        n = s.shape[0]
        ok = np.empty(n, np.uint8)
        nb = np.empty(n, np.int32)
        tot = C.c_size_t()
        lib = load()
        args = (C.byref(self.c_robot), environment.host_handle(), s.ctypes.data_as(_lib.F32P),
                g.ctypes.data_as(_lib.F32P), n, ok.ctypes.data_as(_lib.U8P), nb.ctypes.data_as(_lib.I32P))
        rc = lib.vgpu_cpu_validate_motions_mask(*args, None, 0, C.byref(tot), int(threads))
        if rc != _lib.VGPU_OK and tot.value == 0 and n:
            check(rc)
        blk = np.empty(max(tot.value, 1), np.uint8)
        check(lib.vgpu_cpu_validate_motions_mask(*args, blk.ctypes.data_as(_lib.U8P), blk.size, C.byref(tot),
                                                 int(threads)))
        off = np.concatenate([[0], np.cumsum(nb.astype(np.int64))])
        return ok.astype(bool), nb, blk[:tot.value].astype(bool), off

    def cpu_validate_batch(self, starts, goals, environment: Environment, threads: int = 0):
        """validate_motion of every edge on the CPU rake: (ok, n_e, blocks evaluated)."""
        s = np.ascontiguousarray(starts, np.float32).reshape(-1, self.dimension())
        g = np.ascontiguousarray(goals, np.float32).reshape(-1, self.dimension())
        if s.shape != g.shape:
            raise ValueError("starts and goals differ in shape")
        ok = np.empty(s.shape[0], np.uint8)
        nb = np.empty(s.shape[0], np.int32)
        ne = np.empty(s.shape[0], np.int32)
        check(load().vgpu_cpu_validate_motions(C.byref(self.c_robot), environment.host_handle(),
                                               s.ctypes.data_as(_lib.F32P), g.ctypes.data_as(_lib.F32P), s.shape[0],
                                               ok.ctypes.data_as(_lib.U8P), nb.ctypes.data_as(_lib.I32P),
                                               ne.ctypes.data_as(_lib.I32P), int(threads)))
        return ok.astype(bool), nb, ne

    # --- batches (host numpy in/out) ---
    def sphere_fk_batch(self, q, ctx: Optional[Context] = None) -> np.ndarray:
        ctx = ctx or context()
        q = np.ascontiguousarray(q, np.float32).reshape(-1, self.dimension())
        n = q.shape[0]
        ns = self.n_spheres()
        out = np.empty((3, ns, n), np.float32)
        check(load().vgpu_sphere_fk_host(ctx.h, C.byref(self.c_robot), q.ctypes.data_as(_lib.F32P), n,
                                         out.ctypes.data_as(_lib.F32P)), ctx.h)
        return np.ascontiguousarray(out.transpose(2, 1, 0))

    def fkcc_batch(self, q, environment: Environment, ctx: Optional[Context] = None) -> np.ndarray:
        ctx = ctx or context()
        q = np.ascontiguousarray(q, np.float32).reshape(-1, self.dimension())
        out = np.empty(q.shape[0], np.uint8)
        check(load().vgpu_fkcc_host(ctx.h, C.byref(self.c_robot), environment.handle(ctx),
                                    q.ctypes.data_as(_lib.F32P), q.shape[0], out.ctypes.data_as(_lib.U8P)), ctx.h)
        return out.astype(bool)

    def fkcc_attach_batch(self, q, environment: Environment, ctx: Optional[Context] = None) -> np.ndarray:
        """Robot::fkcc_attach per configuration (robots/panda_base.hh:61-65): the environment's
        attachment posed at each configuration's end effector."""
        ctx = ctx or context()
        q = np.ascontiguousarray(q, np.float32).reshape(-1, self.dimension())
        out = np.empty(q.shape[0], np.uint8)
        check(load().vgpu_fkcc_attach_host(ctx.h, C.byref(self.c_robot), environment.handle(ctx),
                                           q.ctypes.data_as(_lib.F32P), q.shape[0], out.ctypes.data_as(_lib.U8P)),
              ctx.h)
        return out.astype(bool)

    def validate_batch(self, starts, goals, environment: Environment, ctx: Optional[Context] = None):
        ctx = ctx or context()
        s = np.ascontiguousarray(starts, np.float32).reshape(-1, self.dimension())
        g = np.ascontiguousarray(goals, np.float32).reshape(-1, self.dimension())
        if s.shape != g.shape:
            raise ValueError("starts and goals differ in shape")
        ok = np.empty(s.shape[0], np.uint8)
        nb = np.empty(s.shape[0], np.int32)
        check(load().vgpu_validate_motions_host(ctx.h, C.byref(self.c_robot), environment.handle(ctx),
                                                s.ctypes.data_as(_lib.F32P), g.ctypes.data_as(_lib.F32P),
                                                s.shape[0], ok.ctypes.data_as(_lib.U8P),
                                                nb.ctypes.data_as(_lib.I32P)), ctx.h)
        return ok.astype(bool), nb

    # --- batches on device memory (raw pointers, e.g. torch tensor.data_ptr()) ---
    def sphere_fk_device(self, q_ptr: int, n: int, out_ptr: int, ld: int, ctx: Optional[Context] = None):
        ctx = ctx or context()
        check(load().vgpu_sphere_fk(ctx.h, C.byref(self.c_robot), C.c_void_p(q_ptr), n, C.c_void_p(out_ptr), ld),
              ctx.h)

    def sample_fkcc(self, first: int, n: int, environment: Environment, ctx: Optional[Context] = None):
        """Halton<dimension> draws first .. first+n-1 -> scale_configuration -> fkcc, fused on the
        GPU (the PRM sampling stage, prm.hh:236-251).  Returns (q [n, dim], valid [n])."""
        ctx = ctx or context()
        q = np.empty((n, self.dimension()), np.float32)
        ok = np.empty(n, np.uint8)
        check(load().vgpu_sample_fkcc_host(ctx.h, C.byref(self.c_robot), environment.handle(ctx), first, n,
                                           q.ctypes.data_as(_lib.F32P), ok.ctypes.data_as(_lib.U8P)), ctx.h)
        return q, ok.astype(bool)

    def sample_fkcc_device(self, first: int, n: int, environment: Environment, q_ptr: int, valid_ptr: int,
                           ctx: Optional[Context] = None):
        ctx = ctx or context()
        check(load().vgpu_sample_fkcc(ctx.h, C.byref(self.c_robot), environment.handle(ctx), first, n,
                                      C.c_void_p(q_ptr or 0), C.c_void_p(valid_ptr)), ctx.h)

    def fkcc_device(self, q_ptr: int, n: int, environment: Environment, valid_ptr: int,
                    ctx: Optional[Context] = None):
        ctx = ctx or context()
        check(load().vgpu_fkcc(ctx.h, C.byref(self.c_robot), environment.handle(ctx), C.c_void_p(q_ptr), n,
                               C.c_void_p(valid_ptr)), ctx.h)

    def validate_mask_device(self, starts_ptr: int, goals_ptr: int, n: int, environment: Environment, ok_ptr: int,
                             nblocks_ptr: int, block_ok_ptr: int, block_cap: int, ctx: Optional[Context] = None) -> int:
        """Full-mask validate (every rake block evaluated, each block's result kept): returns the
        number of blocks written to block_ok (edge-major, block 0 .. n_e - 1)."""
        ctx = ctx or context()
        total = C.c_size_t()
        check(load().vgpu_validate_motions_mask(ctx.h, C.byref(self.c_robot), environment.handle(ctx),
                                                C.c_void_p(starts_ptr), C.c_void_p(goals_ptr), n, C.c_void_p(ok_ptr),
                                                C.c_void_p(nblocks_ptr or 0), C.c_void_p(block_ok_ptr), block_cap,
                                                C.byref(total)), ctx.h)
        return int(total.value)

    def simplify_device(self, waypoints_ptr: int, capacity: int, len_ptr: int, n_paths: int, environment: Environment,
                        settings: Optional[SimplifySettings] = None, iterations_ptr: int = 0, status_ptr: int = 0,
                        cost_ptr: int = 0, ctx: Optional[Context] = None):
        """vgpu_simplify_paths over device memory: waypoints float32 [n_paths][capacity][dim] and len uint32
        [n_paths] in place; iterations uint32, status uint8 and cost float32 [n_paths] are optional."""
        ctx = ctx or context()
        cs = (settings or SimplifySettings()).c()
        check(load().vgpu_simplify_paths(ctx.h, C.byref(self.c_robot), environment.handle(ctx),
                                         C.c_void_p(waypoints_ptr), int(capacity), C.c_void_p(len_ptr), int(n_paths),
                                         C.byref(cs), C.c_void_p(iterations_ptr or 0), C.c_void_p(status_ptr or 0),
                                         C.c_void_p(cost_ptr or 0)), ctx.h)

    def validate_device(self, starts_ptr: int, goals_ptr: int, n: int, environment: Environment, ok_ptr: int,
                        nblocks_ptr: int = 0, ctx: Optional[Context] = None):
        ctx = ctx or context()
        check(load().vgpu_validate_motions(ctx.h, C.byref(self.c_robot), environment.handle(ctx),
                                           C.c_void_p(starts_ptr), C.c_void_p(goals_ptr), n, C.c_void_p(ok_ptr),
                                           C.c_void_p(nblocks_ptr or 0)), ctx.h)


# robots/panda/fk.hh:113-171 sphere radii (reference order)
_PANDA_RADII = np.array(
    [0.08] + [0.06] * 9 + [0.05, 0.055, 0.055, 0.06, 0.055, 0.055, 0.055, 0.06, 0.06, 0.06, 0.05] + [0.025] * 8 +
    [0.05, 0.05, 0.052, 0.05, 0.025, 0.025, 0.02, 0.02] + [0.028] * 6 + [0.026] * 6 + [0.024] * 6 + [0.012] * 4,
    np.float32)


# robots/fetch/fk.hh:118-228 sphere radii (reference order)
_FETCH_RADII = np.array(
    [0.24, 0.066, 0.22] + [0.066] * 5 + [0.22] + [0.066] * 5 + [0.15] * 6 + [0.07, 0.15] + [0.05] * 5 + [0.03] * 22 +
    [0.055] * 4 + [0.04] * 4 + [0.055] * 6 + [0.03] * 4 + [0.055] + [0.03] * 4 + [0.055] * 3 + [0.03] * 6 +
    [0.055] * 2 + [0.03] * 4 + [0.055] * 2 + [0.05] * 4 + [0.012] * 12 + [0.12] * 6, np.float32)
assert _FETCH_RADII.shape == (111,)


# robots/ur5/fk.hh and robots/baxter/fk.hh sphere radii (reference order)
_UR5_RADII = np.array([0.08, 0.08, 0.08, 0.08, 0.08, 0.08, 0.08, 0.08, 0.06, 0.06, 0.06, 0.06, 0.04, 0.04, 0.04, 0.04, 0.04, 0.04, 0.04, 0.04, 0.04, 0.04, 0.02, 0.015, 0.015, 0.015, 0.02, 0.02, 0.02, 0.02, 0.02, 0.02, 0.02, 0.015, 0.015, 0.015], np.float32)
_BAXTER_RADII = np.array([0.25, 0.25, 0.23, 0.2, 0.1, 0.1, 0.1, 0.08, 0.08, 0.08, 0.1, 0.08, 0.08, 0.08, 0.07, 0.07, 0.07, 0.08, 0.05, 0.1, 0.1, 0.1, 0.08, 0.08, 0.08, 0.1, 0.08, 0.08, 0.08, 0.07, 0.07, 0.07, 0.08, 0.05, 0.5, 0.04, 0.04, 0.015, 0.015, 0.012, 0.012, 0.012, 0.014, 0.014, 0.014, 0.014, 0.015, 0.015, 0.012, 0.012, 0.012, 0.014, 0.014, 0.014, 0.014, 0.04, 0.04, 0.015, 0.015, 0.012, 0.012, 0.012, 0.014, 0.014, 0.014, 0.014, 0.015, 0.015, 0.012, 0.012, 0.012, 0.014, 0.014, 0.014, 0.014], np.float32)


def PandaBase(base_x100: int, base_y100: int, base_z100: int, name: Optional[str] = None) -> Robot:
    """vamp::robots::PandaBase<X100, Y100, Z100> (robots/panda_base.hh:15)."""
    return Robot(name or f"panda_{base_x100}_{base_y100}_{base_z100}", base_x100, base_y100, base_z100)


# robots/panda_grid.hh:10-41 -- including this fork's default Panda at base (2, 2, 0)
panda = PandaBase(200, 200, 0, "panda")
for _i in range(3):
    for _j in range(3):
        globals()[f"panda_{_i}_{_j}"] = PandaBase(100 * _i, 100 * _j, 0, f"panda_{_i}_{_j}")
        __all__.append(f"panda_{_i}_{_j}")


# robots/fetch.hh: vamp::robots::Fetch (8 dof, no base offset)
fetch = Robot("fetch", 0, 0, 0, kind=_lib.VGPU_ROBOT_FETCH)
__all__.append("fetch")


def PandaPair(a100=(0, 0, 0), b100=(100, 0, 0), name: Optional[str] = None) -> Robot:
    """The two-Panda composite of BASELINE configs[4] (14 dof: arm A = PandaBase<a100> on joints
    0..6, arm B = PandaBase<b100> on joints 7..13).  No reference counterpart: validity is
    fkcc_A && fkcc_B && no A-B sphere overlap (oracle/vamp_oracle.c vo_pair_*)."""
    return Robot(name or f"panda_pair_{a100}_{b100}", *a100, kind=_lib.VGPU_ROBOT_PANDA_PAIR, base2=tuple(b100))


panda_pair = PandaPair((0, 0, 0), (100, 0, 0), "panda_pair")
__all__ += ["PandaPair", "panda_pair"]

# robots/ur5.hh (6 dof) and robots/baxter.hh (14-dof dual arm): no base offset
ur5 = Robot("ur5", 0, 0, 0, kind=_lib.VGPU_ROBOT_UR5)
baxter = Robot("baxter", 0, 0, 0, kind=_lib.VGPU_ROBOT_BAXTER)
__all__ += ["ur5", "baxter", "RRTCSettings", "Halton", "PlanningResult", "PRMNeighborParams", "PRMSettings"]
