"""tests/stream_cases.py without a GPU: the table covers every staged call, and its two data sets are what the stream tests
(tests/test_hip_streams.py) assume of them.

COVERAGE.  Every function of the vcrnet_amd modules that carries native._guarded's `__wrapped__`, and every undecorated one of
stream_cases.UNDECORATED (found by reading: it reaches native.call, extension.call_with_workspace or an entry point itself,
or only chains staged calls), is the `covers` of a row or a key of stream_cases.SYNCHRONISES -- which names the source line
that documents the host read.  There is no other exemption: a wrapper added later without a row fails here.

VALIDITY.  make(1) and make(2) of every row have the same keys, shapes, dtypes and scalars and other contents; every
index-typed input lies inside the shared shapes and every CSR triple inside the shared capacity, for both seeds -- so any
mixture of the two sets is a valid input too, and a stale read can change numbers and nothing else."""
import importlib
import inspect
import os

import numpy as np
import pytest

import stream_cases as sc

ROWS = sc.by_name()
PACKAGE = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "vcr-net_amd")


def guarded():
    """"module.function" of every _guarded wrapper defined in a module of the package."""
    import vcrnet_amd  # noqa: F401
    found = set()
    for file in sorted(os.listdir(PACKAGE)):
        if not file.endswith(".py") or file.startswith("_"):
            continue
        module = importlib.import_module("vcrnet_amd." + file[:-3])
        for name, f in vars(module).items():
            if inspect.isfunction(f) and hasattr(f, "__wrapped__") and f.__module__ == module.__name__:
                found.add(f"{file[:-3]}.{name}")
    return found


def resolve(path):
    import vcrnet_amd  # noqa: F401
    head, *rest = path.split(".")
    obj = importlib.import_module("vcrnet_amd." + head)
    for part in rest:
        obj = getattr(obj, part)
    return obj


def test_the_names_of_the_rows_are_unique():
    assert len(ROWS) == len(sc.ROWS)


def test_every_staged_call_is_a_row_or_is_documented_to_synchronise():
    found = guarded()
    assert len(found) >= 71, sorted(found)                   # (the decorator is still what marks them: 71 when written)
    wanted = found | set(sc.UNDECORATED)
    covered = {r.covers for r in sc.ROWS}
    missing = sorted(wanted - covered - set(sc.SYNCHRONISES))
    assert not missing, f"staged calls without a row in tests/stream_cases.py: {missing}"
    both = sorted(covered & set(sc.SYNCHRONISES))
    assert not both, f"a call is either staged or synchronises: {both}"


def test_every_row_and_every_exemption_names_a_function_that_exists():
    for path in {r.covers for r in sc.ROWS} | set(sc.SYNCHRONISES) | set(sc.UNDECORATED):
        assert callable(resolve(path)), path


def test_the_undecorated_list_holds_no_decorated_function():
    assert not set(sc.UNDECORATED) & guarded()


@pytest.mark.parametrize("name", sorted(sc.SYNCHRONISES))
def test_a_call_that_synchronises_says_so_in_its_source(name):
    file, line = sc.SYNCHRONISES[name]
    with open(os.path.join(PACKAGE, file)) as f:
        assert line in f.read(), (name, file)
    assert file.replace(".py", "") == name.split(".")[0]


def test_the_integration_document_lists_the_calls_that_synchronise():
    with open(os.path.join(os.path.dirname(PACKAGE), "INTEGRATION.md")) as f:
        text = f.read()
    for name in sc.SYNCHRONISES:
        assert f"`{name}`" in text, name


@pytest.mark.parametrize("name", list(ROWS))
def test_the_two_data_sets_share_their_shapes_and_differ_in_their_contents(name):
    r = ROWS[name]
    a, b = r.make(1), r.make(2)
    assert list(a) == list(b)
    differ = 0
    for key in a:
        x, y = a[key], b[key]
        if isinstance(x, np.ndarray):
            assert isinstance(y, np.ndarray) and x.shape == y.shape and x.dtype == y.dtype, key
            assert x.size > 0 and x.dtype != object, key
            if x.dtype.kind == "f":
                assert not np.isnan(x).any() and not np.isneginf(x).any(), key             # (+inf pads a d2 list)
                assert not np.array_equal(x, y), f"{key}: the same values at both seeds"
            differ += not np.array_equal(x, y)
        else:
            assert type(x) is type(y) and x == y, f"{key}: a scalar argument differs between the seeds"
    assert differ >= 1
    assert r.make(1) is a                                    # computed once, shared


@pytest.mark.parametrize("name", [n for n, r in ROWS.items() if r.ranges or r.csr])
def test_the_index_inputs_lie_inside_the_shared_shapes(name):
    r = ROWS[name]
    for seed in (1, 2):
        kw = r.make(seed)
        for key, (lo, hi) in r.ranges.items():
            v = kw[key]
            assert v.dtype.kind == "i" and lo <= v.min() and v.max() < hi, (seed, key, int(v.min()), int(v.max()), lo, hi)
        for idx, row_start, total in r.csr:
            capacity = kw[idx].shape[1]
            start, tot = kw[row_start], kw[total]
            assert start.dtype == np.int64 and tot.dtype == np.int64
            assert (start[:, 0] == 0).all() and (np.diff(start, axis=1) >= 0).all(), seed
            assert (start[:, -1] == tot).all() and (tot <= capacity).all() and (tot > 0).all(), (seed, tot, capacity)
            if kw[idx].dtype.kind == "i":                     # an index list: every slot, the ones behind the total too
                assert kw[idx].dtype == np.int32 and idx in r.ranges


def test_every_integer_array_of_a_row_that_indexes_is_declared():
    """An int32 / int64 input is an index, a CSR offset, a flag or a histogram: the first two are declared, the last two are
    read as values.  (Listed here so that a new row has to say which.)"""
    values = {"mask", "inlier", "keypoint", "flag", "frame", "sizes", "spfh", "support_spfh", "centre_spfh", "uncertain",
              "w_planes", "row_start", "total"}
    for r in sc.ROWS:
        for key, v in r.make(1).items():
            if isinstance(v, np.ndarray) and v.dtype.kind in "iu":
                assert key in r.ranges or key in values, (r.name, key)


def test_the_rows_take_more_than_one_workgroup_and_end_ragged():
    assert sc.B >= 2 and sc.N > 256 and sc.N % 256 and sc.M > 256 and sc.M % 256 and sc.NS > 256 and sc.NS % 64
    x = sc.cloud(1)
    assert not np.array_equal(x[0], x[1])                    # the clouds of a batch differ
