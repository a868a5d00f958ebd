"""The split policy of the five entry points that cut a brute-force scan into segments, without a GPU: over the grid of
tests/golden/gen_scan_forms.py (shapes at the block and segment edges, three CU counts, every forced Q and S, the refusals
included) the library answers what tests/golden/scan_forms.json recorded at the commit before csrc/seg_scan.h took the policy
over -- not what the code under test computes."""
import json
import os
import sys

import numpy as np
import pytest

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
sys.path.insert(0, GOLDEN)
import gen_scan_forms as gen  # noqa: E402


@pytest.fixture(scope="module")
def recorded():
    import vcrnet_amd  # noqa: F401
    from vcrnet_amd import build
    build.build()
    with open(gen.PATH) as fh:
        return json.load(fh)


def test_the_file_holds_the_grid_the_generator_walks(recorded):
    assert recorded["grid"] == gen.GRID and set(recorded["entries"]) == set(gen.ENTRIES)
    points = {"vcr_nn_score": 54000, "vcr_refine": 54000, "vcr_voxel": 4500, "vcr_outlier_radius": 4500, "vcr_feat_nn": 108000}
    for name, e in gen.ENTRIES.items():
        assert recorded["entries"][name]["axes"] == list(e.axes) and recorded["entries"][name]["rows"] == points[name], name


@pytest.mark.parametrize("name", sorted(gen.ENTRIES))
def test_the_library_reproduces_the_recorded_forms(recorded, name):
    want = gen.decode(recorded["entries"][name]["data"])
    got = gen.answers(name)
    assert want.shape == got.shape == (recorded["entries"][name]["rows"], 4)
    assert (want[:, 0] == 0).any() and (want[:, 0] == -1).any() and (want[:, 0] == -3).any()    # served, EINVAL, EUNSUPPORTED
    differ = np.flatnonzero((want != got).any(axis=1))
    if len(differ):
        at = differ[0]
        point = dict(zip(gen.ENTRIES[name].axes, list(gen.ENTRIES[name].points())[at]))
        pytest.fail(f"{name}: {len(differ)} of {len(want)} grid points differ; the first, {point}: recorded (rc, Q, S, bytes) = "
                    f"{want[at].tolist()}, the library answers {got[at].tolist()}")
