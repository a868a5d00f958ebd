"""Every staged call on a side stream and under HIP graph capture (the table: tests/stream_cases.py; its coverage and the
validity of its inputs: tests/test_stream_table_cpu.py).  INTEGRATION.md promises of every C entry point and of the staged
Python call in front of it: asynchronous on the caller's stream, no allocation by the library, no synchronisation.  The other
GPU files run on the legacy default stream, which orders every launch of the process: a launch that lost its stream argument,
a torch op a wrapper issues elsewhere, a launch decision taken from a value read on the host are all invisible there.

THE REFERENCE of every check is the same call, eager, on the default stream, on the same inputs, followed by
torch.cuda.synchronize().  The comparison is torch.equal on the outputs' BYTES: the files of the operations tie that reference to
the restatements, every call repeats itself bit for bit, and a NaN padding equals itself.  No tolerance.

(a) ORDERED ON A SIDE STREAM.  The input buffers hold data set A.  On a side stream (one the default stream is seen not to queue
    behind: independent_stream): a device-side delay (torch.cuda._sleep),
    then the copy of data set B into the buffers, then the call.  On return the stream must still be busy (query() is False: every
    launch was issued while the buffers held A -- otherwise the test FAILS and says the delay is too short), and after its
    synchronisation the outputs must be the reference for B.  A launch on any other stream ran during the delay and read A.
(b) CAPTURE AND REPLAY ON OTHER DATA.  A warm-up call on the capture stream (hipFuncSetAttribute, the CU-count cache), one call
    captured on buffers that hold A, then B copied in and two replays (the reference for B), A copied back and a replay (the
    reference for A).  A call that allocates through the runtime or synchronises makes the capture raise; a launch that was not
    captured, or a launch parameter the host took from A, shows as a replay that does not follow its inputs.  The captured region
    is one single-stream chain: the wrappers hold torch.empty (and, in icp and knn_pair_deferred, a torch.zeros: a fill KERNEL,
    not a memset node) and the C calls; `prefill` stays None.
(c) THE PUBLIC COMPOSITE CALLS (stream_cases.COMPOSITES) are documented to synchronise at most once, so they get the WEAKER
    check: (a) without the query() condition -- a call that waits for the device has let the delay pass by the time it returns
    -- and no capture.  A launch on another stream before the first synchronisation still reads A and still fails.
(d) THE HARNESS TESTS ITSELF on fake staged calls in plain torch: one runs an op on a stream of its own -- (a) must report
    a mismatch and (b) a replay that does not follow its inputs --, one reads a device scalar with .item() -- the capture must
    raise --, and on a real wrapper handed the NULL stream, which (b) must refuse or expose.  Without them a green run of (a)
    and (b) would prove nothing about the harness.  (a) is evidence against launches on other streams; against a stray null
    stream the check is (b).

THE DELAY.  Measured on an MI355X (time.perf_counter() around each row's eager call, no synchronisation, second call of each):
the slowest enqueue of the table is MEASURED_ENQUEUE_MS below; the delay is ten times that, rounded up.  The sleep is given in
clock ticks, so the ticks of a millisecond are measured once a run."""
import functools
import time

import numpy as np
import pytest
import torch

import stream_cases as sc

pytestmark = pytest.mark.gpu

MEASURED_ENQUEUE_MS = 0.340              # the slowest row's host time (farthest_point_sample)
DELAY_MS = 3.5                             # >= 10 x MEASURED_ENQUEUE_MS

ROWS = sc.by_name()
COMPOSITES = {c.name: c for c in sc.COMPOSITES}


# ---------------------------------------------------------------------------------------------------------------- the harness

def on_device(kw):
    """Host arrays -> fresh device tensors (the static buffers); scalars as they are."""
    return {k: torch.from_numpy(np.ascontiguousarray(v)).cuda() if isinstance(v, np.ndarray) else v for k, v in kw.items()}


def tensors(out, at=""):
    """Every tensor of a call's result, by its path: dicts, tuples and lists are walked, anything else is left out."""
    if torch.is_tensor(out):
        return {at: out}
    found = {}
    if isinstance(out, dict):
        for k, v in out.items():
            found.update(tensors(v, f"{at}.{k}" if at else str(k)))
    elif isinstance(out, (tuple, list)):
        for i, v in enumerate(out):
            found.update(tensors(v, f"{at}[{i}]"))
    return found


def kept(out):
    return {k: v.clone() for k, v in tensors(out).items()}


def wrong(got, want):
    """The outputs of `got` that are not `want`'s, byte for byte."""
    assert list(got) == list(want), (list(got), list(want))
    bad = []
    for k in want:
        a, b = got[k], want[k]
        if a.shape != b.shape or a.dtype != b.dtype or not torch.equal(a.contiguous().view(-1).view(torch.uint8),
                                                                       b.contiguous().view(-1).view(torch.uint8)):
            bad.append(k)
    return bad


@functools.lru_cache(maxsize=None)
def ticks_per_ms():
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda._sleep(1000)
    torch.cuda.synchronize()
    a.record()
    torch.cuda._sleep(4_000_000)
    b.record()
    b.synchronize()
    return 4_000_000 / a.elapsed_time(b)


def eager(call, kw):
    """The reference: the call on the default stream, then the device drained."""
    out = kept(call(**on_device(kw)))
    torch.cuda.synchronize()
    return out


@functools.lru_cache(maxsize=None)
def reference(table, name, seed):
    case = (ROWS if table == "rows" else COMPOSITES)[name]
    return eager(case.call, case.make(seed))


def enqueue_ms(name):
    """Host time of the row's eager call without a synchronisation: the slowest of five, after a first call that loads and
    plans.  `python tests/test_hip_streams.py` on the GPU prints it for every row and the slowest, which is where
    MEASURED_ENQUEUE_MS comes from when rows are added."""
    r = ROWS[name]
    kw = on_device(r.make(1))
    r.call(**kw)
    slowest = 0.0
    for _ in range(5):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        r.call(**kw)
        slowest = max(slowest, time.perf_counter() - t0)
    torch.cuda.synchronize()
    return slowest * 1e3


def independent_stream(delay_ms=DELAY_MS):
    """A stream of torch's pool that the legacy default stream does not queue behind: a delay on the stream, one op on the default
    stream, and that op must finish while the stream is still busy.  The runtime deals its streams onto a few hardware queues
    (four here), and two streams that share one run in the order of their launches: behind a side stream that shared the
    default stream's queue a launch that went to the default stream would wait for the overwrite and pass.
    THE LIMIT OF CHECK (a): it sees a launch on a stream that runs beside the side stream -- the fake below.  It is not relied
    on for a launch on the NULL stream: whether that one waits for the side stream is the runtime's business, and this probe
    speaks for torch's own launches only.  That case is held by check (b): a launch on the legacy stream cannot be recorded
    into another stream's capture (test_the_capture_check_reports_an_entry_point_launched_on_the_null_stream)."""
    probe = torch.zeros(1, device="cuda")
    for _ in range(64):                                      # (the pool hands out 32 streams in turn)
        s = torch.cuda.Stream()
        torch.cuda.synchronize()
        with torch.cuda.stream(s):
            torch.cuda._sleep(int(delay_ms * ticks_per_ms()))
        probe.add_(1.0)
        done = torch.cuda.Event()
        done.record()
        done.synchronize()
        free = not s.query()
        torch.cuda.synchronize()
        if free:
            return s
    pytest.fail("no stream of the pool runs beside the default stream: check (a) could not see a launch on the null stream")


def side_stream(call, a, b, delay_ms=DELAY_MS):
    """Check (a) -> (busy, outputs): the buffers hold a; on a side stream the delay, the copy of b, the call."""
    x, fresh = on_device(a), on_device(b)
    side = independent_stream(delay_ms)
    torch.cuda.synchronize()
    with torch.cuda.stream(side):
        torch.cuda._sleep(int(delay_ms * ticks_per_ms()))
        for k, v in fresh.items():
            if torch.is_tensor(v):
                x[k].copy_(v)
        out = call(**x)
        busy = not side.query()
        side.synchronize()
        out = kept(out)
    torch.cuda.synchronize()
    return busy, out


def captured(call, a, b):
    """Check (b) -> the outputs of (replay on b, second replay on b, replay on a)."""
    x, first, second = on_device(a), on_device(a), on_device(b)
    torch.cuda.synchronize()
    g, st = torch.cuda.CUDAGraph(), torch.cuda.Stream()
    with torch.cuda.stream(st):
        call(**x)                                            # first-call work happens outside the capture
        st.synchronize()
        with torch.cuda.graph(g, stream=st):
            out = call(**x)
    torch.cuda.synchronize()
    results = []
    for data, replays in ((second, 2), (first, 1)):
        for k, v in data.items():
            if torch.is_tensor(v):
                x[k].copy_(v)
        for _ in range(replays):
            g.replay()
            torch.cuda.synchronize()
            results.append(kept(out))
    return results


# ---------------------------------------------------------------------------------------------- (d) the harness tests itself

class OffStream:
    """A fake staged call, z = 2 x + y into buffers of its own, whose doubling runs on ANOTHER stream and is never waited for:
    the bug the checks are there to find.  Plain torch ops on valid buffers."""

    def __init__(self, n):
        self.other = torch.cuda.Stream()
        self.tmp, self.z = torch.zeros(n, device="cuda"), torch.zeros(n, device="cuda")
        with torch.cuda.stream(self.other):                  # a stream in use: its first launch, which sets it up, is behind it
            self.tmp.zero_()
        self.other.synchronize()

    def __call__(self, x, y):
        with torch.cuda.stream(self.other):
            torch.mul(x, 2.0, out=self.tmp)
        torch.add(self.tmp, y, out=self.z)
        return {"z": self.z}


def host_branch(x, y):
    """A fake staged call that reads a device scalar on the host to pick its launch."""
    return {"z": x + y if x.sum().item() > 0 else x - y}


def waits(x, y):
    """A fake staged call that waits for its own result."""
    z = x + y
    z[0].item()
    return {"z": z}


def fake_data(seed, n=1 << 16):
    rs = np.random.RandomState(seed)
    return {"x": rs.uniform(1.0, 2.0, n).astype(np.float32), "y": rs.uniform(1.0, 2.0, n).astype(np.float32)}


def fake_reference(kw):
    return {"z": torch.from_numpy(np.float32(2.0) * kw["x"] + kw["y"]).cuda()}


def test_the_side_stream_check_reports_an_op_on_another_stream():
    a, b = fake_data(1), fake_data(2)
    fake = OffStream(len(a["x"]))
    fake(**on_device(a))                                     # (a first call loads the kernels: the rows' reference does the same)
    torch.cuda.synchronize()
    busy, out = side_stream(fake, a, b)
    fake.other.synchronize()
    assert busy
    assert wrong(out, fake_reference(b)) == ["z"]            # the doubling read A during the delay
    busy, out = side_stream(lambda x, y: {"z": 2.0 * x + y}, a, b)
    assert busy and not wrong(out, fake_reference(b))        # the same arithmetic on the caller's stream passes


def test_the_side_stream_check_sees_a_delay_that_is_too_short():
    a, b = fake_data(1), fake_data(2)
    busy, out = side_stream(waits, a, b)                     # (.item() waits for the stream: it is idle on return)
    assert not busy
    assert not wrong(out, {"z": torch.from_numpy(b["x"] + b["y"]).cuda()})


def test_the_capture_check_reports_a_replay_that_does_not_follow_its_inputs():
    a, b = fake_data(1), fake_data(2)
    fake = OffStream(len(a["x"]))
    on_b, again, on_a = captured(fake, a, b)
    assert wrong(on_b, fake_reference(b)) == ["z"] and wrong(again, fake_reference(b)) == ["z"]
    assert not wrong(on_a, fake_reference(a))                # (what the capture-time launch left behind fits A)
    on_b, again, on_a = captured(lambda x, y: {"z": 2.0 * x + y}, a, b)
    assert not wrong(on_b, fake_reference(b)) and not wrong(again, fake_reference(b)) and not wrong(on_a, fake_reference(a))


def test_the_delay_is_ten_times_the_slowest_measured_enqueue():
    assert DELAY_MS >= 10.0 * MEASURED_ENQUEUE_MS > 0.0


# ------------------------------------------------------------------------------------------------------- (a), (b): the rows

@pytest.mark.parametrize("name", list(ROWS))
def test_a_staged_call_is_ordered_on_a_side_stream(name):
    r = ROWS[name]
    want = reference("rows", name, 2)
    assert tuple(want) == r.outputs
    busy, out = side_stream(r.call, r.make(1), r.make(2))
    assert busy, f"{name}: the side stream was idle when the call returned -- the delay of {DELAY_MS} ms is too short, or the call waits"
    bad = wrong(out, want)
    assert not bad, f"{name}: {bad} differ from the eager call on the same inputs -- a launch outside the caller's stream read the old data"


@pytest.mark.parametrize("name", list(ROWS))
def test_a_staged_call_captures_into_a_graph_that_follows_its_inputs(name):
    r = ROWS[name]
    on_b, again, on_a = captured(r.call, r.make(1), r.make(2))
    bad = wrong(on_b, reference("rows", name, 2)), wrong(again, reference("rows", name, 2)), wrong(on_a, reference("rows", name, 1))
    assert not any(bad), f"{name}: replays on (B, B again, A) differ from the eager calls in {bad}"


# ----------------------------------------------------------------------------------------------- (c): the public composites

@pytest.mark.parametrize("name", list(COMPOSITES))
def test_a_public_call_reads_what_its_stream_wrote(name):
    """The weaker check: these calls may synchronise once (search_radius with capacity=None reads the largest total back, ISS its
    default radii, register_sampled its counts), so the stream may be idle when they return and a graph could not hold them."""
    c = COMPOSITES[name]
    _, out = side_stream(c.call, c.make(1), c.make(2))
    bad = wrong(out, reference("composites", name, 2))
    assert not bad, f"{name}: {bad} differ from the eager call on the same inputs"


# ----------------------------------------------------------------------------------------------- (d), last: broken captures

def test_the_capture_check_reports_an_entry_point_launched_on_the_null_stream(monkeypatch):
    """The bug the file is about, planted in a real wrapper: native.call hands the entry point the null stream instead of the
    caller's.  The eager call on the default stream does not show it; the capture must raise, or its replays must not follow B."""
    import vcrnet_amd  # noqa: F401
    from vcrnet_amd import native
    r = ROWS["to_rows4"]
    on_a, on_b = reference("rows", "to_rows4", 1), reference("rows", "to_rows4", 2)
    monkeypatch.setattr(native, "stream_ptr", lambda device=None: 0)
    assert not wrong(eager(r.call, r.make(2)), on_b)         # invisible where the other GPU files run
    try:
        first, again, _ = captured(r.call, r.make(1), r.make(2))
    except RuntimeError:                                     # (VcrHipError is one: the entry point's launch was refused)
        pass
    else:
        assert wrong(first, on_b) == ["rows"] and wrong(again, on_b) == ["rows"]
        assert not wrong(first, on_a)                        # what the launch outside the graph left behind
    torch.cuda.synchronize()
    monkeypatch.undo()
    assert not wrong(eager(r.call, r.make(2)), on_b)         # the process goes on


def test_the_capture_check_raises_on_a_host_read():
    a, b = fake_data(1), fake_data(2)
    with pytest.raises(RuntimeError):
        captured(host_branch, a, b)
    torch.cuda.synchronize()
    assert torch.ones(4, device="cuda").sum().item() == 4.0  # the process goes on


if __name__ == "__main__":
    import os
    import sys
    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))        # (what tests/conftest.py does)
    times = {name: enqueue_ms(name) for name in ROWS}
    for name, ms in times.items():
        print(f"{ms:8.3f} ms  {name}")
    slowest = max(times, key=times.get)
    print(f"slowest enqueue {times[slowest]:.3f} ms ({slowest}); DELAY_MS = {DELAY_MS}, MEASURED_ENQUEUE_MS = {MEASURED_ENQUEUE_MS}")
