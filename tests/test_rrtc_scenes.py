"""The multi-scene batched RRT-Connect entry points (vgpu_rrtc_batch_scenes, Robot.rrtc_batch_scenes) without a
GPU: the exports and their signatures, the new kernel's registers, the argument checks made before any device call,
and a clean error where no device exists.  What the kernel computes is tests/test_gpu_rrtc_scenes.py's subject."""
import ctypes
import os
import sys

import numpy as np
import pytest

from conftest import ROOT
from test_rrtc_batch import HEADER, LIB, declaration

# the parameter types the ABI declares, in order
SCENES = ["vgpu_ctx *", "const vgpu_robot *", "vgpu_env *const *", "size_t", "const uint32_t *", "const float *",
          "const float *", "size_t", "size_t", "const vgpu_rrtc_settings *", "uint64_t *", "size_t", "float *", "size_t",
          "uint32_t *", "vgpu_plan_result *", "uint8_t *"]
DECLARED = {"vgpu_rrtc_batch_scenes": SCENES, "vgpu_rrtc_batch_scenes_host": SCENES}


@pytest.mark.parametrize("name", sorted(DECLARED))
def test_exports_are_declared(name):
    with open(HEADER) as f:
        assert declaration(f.read(), name) == DECLARED[name]


@pytest.mark.parametrize("name", sorted(DECLARED))
def test_library_exports_and_bindings(name):
    from vamp_amd import _lib
    lib = _lib.load()
    assert hasattr(lib, name)
    res, args = _lib.SIGNATURES[name]
    assert res is ctypes.c_int and len(args) == len(DECLARED[name])
    for a, t in zip(args, DECLARED[name]):  # sizes by value, everything else a pointer
        if t == "size_t":
            assert a is ctypes.c_size_t
        else:
            assert a is ctypes.c_void_p or issubclass(a, ctypes._Pointer)
    # the single-scene calls keep their signatures
    assert len(_lib.SIGNATURES["vgpu_rrtc_batch"][1]) == len(_lib.SIGNATURES["vgpu_rrtc_batch_host"][1]) == 15


def test_python_entry_points():
    import inspect

    import vamp_amd as vamp
    names = list(inspect.signature(vamp.Robot.rrtc_batch_scenes).parameters)
    assert names == ["self", "starts", "goals", "environments", "env_index", "settings", "rng_first", "node_cap",
                     "path_cap", "ctx", "slice"]
    assert hasattr(vamp.Robot, "rrtc_scenes_device")


def test_scenes_kernel_does_not_spill():
    """the primitive-environment instantiation of the multi-scene kernel: 0 scratch and 0 VGPR spills (AMDGPU
    metadata note of the built library, tools/kernel_resources.py); both instantiations are there, and their names
    stay clear of the single-scene kernel's"""
    if not os.path.exists(LIB):
        pytest.skip("libvampgpu.so not built (make -C mr-vamp_amd)")
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import kernel_resources
    ks = [k for k in kernel_resources.kernels(LIB) if "rrtc_scenes_kernel<" in k["name"]]
    prim = [k for k in ks if "rrtc_scenes_kernel<false>" in k["name"]]
    assert len(prim) == 1 and any("rrtc_scenes_kernel<true>" in k["name"] for k in ks), [k["name"][:60] for k in ks]
    assert not any("vgpu::rrtc_kernel<" in k["name"] for k in ks)
    print(f"rrtc_scenes_kernel<false>: vgpr {prim[0]['vgpr']} scratch {prim[0]['scratch']} "
          f"spills {prim[0]['vgpr_spill']}")
    assert prim[0]["scratch"] == 0 and prim[0]["vgpr_spill"] == 0, prim[0]


class NoDevice:
    """an Environment and a Context stand-in that fail the test if a device call is attempted"""

    def handle(self, ctx):
        raise AssertionError("the environment was realised: a device call before the argument check")

    @property
    def h(self):
        raise AssertionError("the context was used before the argument check")


@pytest.mark.parametrize("n_envs,env_index", [(3, None), (1, None), (2, [0, 1, 0]), (2, [[0, 1], [0, 1]]), (4, [0]),
                                              (4, [0, 1, 2, -1]), (4, [0, 1, 2, 2 ** 32])],
                         ids=["default-needs-P-envs", "default-one-env", "short", "shape", "one-entry", "negative",
                              "over-32-bits"])
def test_env_index_is_checked_before_any_device_call(n_envs, env_index):
    """P = 4: without env_index the list must hold P environments; with it, one entry per problem, each an unsigned
    32-bit number.  ValueError, with neither the context nor an environment touched"""
    import vamp_amd as vamp
    q = np.zeros((4, 7), np.float32)
    stub = NoDevice()
    with pytest.raises(ValueError):
        vamp.panda_0_0.rrtc_batch_scenes(q, q, [stub] * n_envs, env_index, ctx=stub)


def test_rrtc_batch_scenes_raises_without_a_device():
    """no device: a VgpuError from the context, nothing else (where there is a device this has nothing to check)"""
    import vamp_amd as vamp
    try:
        vamp.context()
    except vamp.VgpuError:
        q = np.zeros((2, 7), np.float32)
        with pytest.raises(vamp.VgpuError):
            vamp.panda_0_0.rrtc_batch_scenes(q, q, [vamp.Environment(), vamp.Environment()])
        with pytest.raises(vamp.VgpuError):
            vamp.panda_0_0.rrtc_batch_scenes(q, q, [vamp.Environment()], [0, 0])
