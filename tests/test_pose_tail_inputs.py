"""The inputs of tests/test_hip_pose_tail.py, checked on the CPU with the references alone: for every case of
tests/pose_tail_cases.py the fp32 oracle and its float64 twin are run and the conditions the kernel tests rely on are asserted
-- so that a kernel test that fails there fails because of the kernel, not because its input sat on a decision boundary."""
import numpy as np
import pytest

import pose_tail_cases as C


@pytest.mark.parametrize("name", [c.name for c in C.RIGID_CASES])
def test_rigid_reference_meets_what_the_kernel_is_held_to(name):
    """Assertions (a) and (b) of the kernel test hold for the twin's own R (so they ask nothing a correct solve cannot give),
    and the fp32 reference stays finite."""
    ref = C.rigid_reference(name)
    B = C.RIGID[name].B
    assert all(np.isfinite(ref[k]).all() for k in ("R32", "t32", "H32", "R64", "t64", "H64"))
    R = ref["R64"]
    assert np.abs(R @ R.transpose(0, 2, 1) - np.eye(3)).max() <= 1e-12 and np.abs(np.linalg.det(R) - 1).max() <= 1e-12
    assert np.all(np.einsum("bij,bji->b", R, ref["H64"]) >= ref["opt"] - 1e-12 * ref["s1"])
    assert ref["margin"].shape == (B,)


def test_only_the_named_rigid_cases_may_be_ill_determined():
    """Rule (c)'s precondition s2 + d s3 >= 1e-3 s1, on every sample: whichever case misses it gets (a) and (b) only, and no
    case but the two named ones may."""
    ill = [c.name for c in C.RIGID_CASES if not C.well_determined(c.name)]
    assert set(ill) <= set(C.MAY_BE_ILL), ill
    for fam in {c.family for c in C.RIGID_CASES}:
        assert all(np.isfinite(C.rigid_family_floor(fam)))


def test_rigid_cases_reach_the_branches_they_are_named_for():
    d = lambda n: C.rigid_reference(n)["d"]
    assert (d("mirror_noisy") < 0).all()                                    # every sample takes the reflection rule
    assert (d("flat_source") < 0).any() and (d("flat_source") > 0).any()    # some do, some do not
    tw = C.rigid_reference("twelve_points")
    S = np.linalg.svd(tw["H64"], compute_uv=False)
    assert np.abs(S[:, 2] / S[:, 0] - 1).max() <= 1e-6 and (tw["d"] > 0).all()       # three equal singular values, R unique
    assert (tw["H64"][:3] == 0).sum() == 18                                 # quarter turns: six exact zeros each
    r2 = np.linalg.svd(C.rigid_reference("rank2_tilted")["H64"], compute_uv=False)
    ratio = r2[:, 2] / r2[:, 0]
    assert (ratio > 1e-12).all() and (ratio < 1e-6).all()                   # rank 2 up to fp32 rounding: no completion
    assert sorted({c.K for c in C.RIGID_CASES if c.name.startswith("K")}) == [3, 4, 63, 64, 65, 255, 256, 257, 511, 1000, 4099]


@pytest.mark.parametrize("name", list(C.ICP_SPECS))
def test_icp_inputs_are_free_of_near_ties(name):
    """On the twin's run: in every iteration every source point's best score leads the second best by >= 32 * 2^-24 * P, and
    | |prev - err| - tolerance | >= the same margin -- neither a neighbour nor the stop can turn on an fp32 rounding.  The
    restated loop is the oracle's (same error trace), and the fp32 reference stops where the twin does."""
    c = C.icp_case(name)
    errs, gap, stop, P = C.icp_preconditions(c.src.double(), c.tgt.double(), c.max_it, c.tol)
    ref = C.icp_reference(name)
    assert len(errs) == ref["iters64"] == ref["iters32"]
    assert gap >= C.MARGIN * P, (gap, C.MARGIN * P)
    assert stop >= C.MARGIN * P, (stop, C.MARGIN * P)
    assert (c.B, c.N, c.M) == {"I1": (3, 300, 2197), "I2": (3, 300, 2197), "I3": (2, 513, 4913), "I4": (5, 77, 125),
                               "I5": (2, 100, 216), "I6": (3, 300, 2197), "I7": (2, 150, 2197), "I8": (2, 50, 1)}[name]


def test_icp_cases_reach_what_they_are_named_for():
    it = {n: C.icp_reference(n)["iters32"] for n in C.ICP_SPECS}
    assert 1 < it["I2"] < it["I1"] < 30                                     # both stop before the limit, I2 earlier
    assert it["I3"] == 6 and it["I5"] == 1 and it["I6"] == 1 and 1 < it["I7"] < 30 and it["I4"] < 30 and it["I8"] < 10
    i3 = C.icp_case("I3")                                                   # nearest neighbours in every candidate tile
    first = C.oracle.neg_sqdist_head(i3.src.double(), i3.tgt.double()).argmax(-1).numpy()
    assert all(((first >= lo) & (first < lo + 2048)).mean() > 0.1 for lo in (0, 2048, 4096))
    eye = np.broadcast_to(np.eye(3), (2, 3, 3))
    assert np.abs(C.icp_reference("I5")["R32"] - eye).max() <= 1e-6
    assert np.abs(C.icp_reference("I8")["R32"] - eye).max() <= 1e-6         # H = 0 exactly in the reference's loop too
    i7 = C.icp_reference("I7")                                              # pair 0 starts aligned, pair 1 does not
    ang = lambda R: np.degrees(np.arccos(np.clip((np.trace(R) - 1) / 2, -1, 1)))
    assert ang(i7["R64"][0]) < 0.1 and ang(i7["R64"][1]) > 5


def test_pose_inputs():
    for B, N in C.POSE_SHAPES:
        p = C.pose_inputs(B, N)
        assert p.cloud.shape == (B, 3, N) and float(p.t1.abs().max()) > 100 and float(p.t1.abs().max()) <= 1e3
        R = p.R1.double().numpy()
        assert np.abs(R @ R.transpose(0, 2, 1) - np.eye(3)).max() <= 1e-6
