"""The roadmap neighbour query on the GPU with caller-chosen k, r and kmax (vgpu_roadmap_knn_range), against the
plain loop (oracle_py.roadmap_knn_kr) on the cases of tests/knn_cases.py, by the brute-force kernels (mode 1:
knn_kernel, knn_merge_kernel) and by the spatial index (mode 2: group_kernel; under the variant settings also
query_kernel, coop_kernel and the coded group_kernel).  The lists are the project's exact contract: cnt equal,
nbr and dist bit for bit on the first cnt slots.  Every call writes between sentinel guard rows that must come
back untouched, with cnt <= kmax (knn_probe.knn_gpu_kr): a k[i] above kmax is treated as kmax."""
import os
import subprocess
import sys

import numpy as np
import pytest

import knn_cases
import knn_probe

pytestmark = pytest.mark.gpu
HERE = os.path.dirname(os.path.abspath(__file__))
MODES = {"brute": 1, "index": 2}

# the index's kernel variants (vgpu_knn_index.hip), one fresh process each
VARIANTS = {
    "group0": {"VAMP_AMD_KNN_GROUP": "0"},
    "group1": {"VAMP_AMD_KNN_GROUP": "1"},
    "group2": {"VAMP_AMD_KNN_GROUP": "2"},
    "group8": {"VAMP_AMD_KNN_GROUP": "8"},
    "coop4": {"VAMP_AMD_KNN_COOP": "4"},
    "coop8": {"VAMP_AMD_KNN_COOP": "8"},
    "qcode": {"VAMP_AMD_KNN_QCODE": "1"},
    "qcode_group1": {"VAMP_AMD_KNN_QCODE": "1", "VAMP_AMD_KNN_GROUP": "1"},
}


@pytest.fixture(scope="module")
def vamp():
    import vamp_amd
    assert vamp_amd.context(0) is not None
    return vamp_amd


@pytest.mark.parametrize("mode", list(MODES))
@pytest.mark.parametrize("name", knn_cases.SMALL)
def test_knn_equals_oracle(vamp, oracle, name, mode):
    case = knn_cases.get(name)
    for i, got in enumerate(knn_probe.run_case(vamp, case, MODES[mode])):
        knn_cases.same_lists(got, case.ref(i), case.kmax)


@pytest.mark.parametrize("mode", ["index", "brute"])
def test_more_than_64_super_tiles(vamp, oracle, mode):
    """n = 300000: the index's outward loop over chunks of 64 super-tiles takes more than one chunk; a cluster in
    the middle of the Halton vertices; only two ranges of 512 queries, so the brute force stays small too"""
    case = knn_cases.get("super-d8")
    for i, got in enumerate(knn_probe.run_case(vamp, case, MODES[mode])):
        knn_cases.same_lists(got, case.ref(i), case.kmax)


def test_variants_equal_oracle(oracle, tmp_path):
    """every shipped variant of the index query gives the oracle's lists on the PROBE cases; the children run
    strictly one after another, and the first that fails ends the test"""
    cases = [knn_cases.get(name) for name in knn_cases.PROBE]
    inp = str(tmp_path / "inputs.npz")
    knn_probe.save_inputs(inp, cases)
    for vname, extra in VARIANTS.items():
        out = str(tmp_path / f"{vname}.npz")
        env = {k: v for k, v in os.environ.items() if not k.startswith("VAMP_AMD_KNN_")}
        env.update(extra)
        r = subprocess.run([sys.executable, os.path.join(HERE, "knn_probe.py"), inp, out], env=env,
                           capture_output=True, text=True, timeout=120)
        assert r.returncode == 0, (vname, r.stderr[-2000:])
        got = np.load(out, allow_pickle=False)
        for case in cases:
            for i in range(len(case.ranges)):
                try:
                    knn_cases.same_lists([got[f"{case.name}/{i}/{key}"] for key in ("nbr", "dist", "cnt")],
                                         case.ref(i), case.kmax)
                except AssertionError as e:
                    raise AssertionError(f"variant {vname} {extra}, case {case.name}, range {i}: {e}") from None
        print(f"knn variant {vname}: {extra} -> the oracle's lists", flush=True)
