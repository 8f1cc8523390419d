"""The harness of tests/test_launch_contract_gpu.py: does every kernel and memset of an engine call run on
the caller's stream, of the device that holds the tensors, without a wait on the host?

On torch's default stream everything is ordered anyway, so a launcher that passed 0 instead of its stream
for one of its kernels or memsets passes every value test that runs there.  The protocol below makes the
order matter.  On a side stream `s` a device-side delay of about 0.1 s is enqueued first, then the copy of
the true inputs into staging buffers that hold a decoy (other valid spectra), then the fill of every output
with a sentinel, then the call under test on the staging buffers.  A kernel or memset of the call that was
enqueued anywhere but on `s` runs while `s` still sleeps: it reads the decoy, or what it writes is
overwritten by the sentinel fill, and the outputs differ from the reference bits.  A call that waits on the
host shows as a stream that is idle when the call returns.

Nothing here is a test; the module keeps the calibrated delay of each device for the session.
"""
import contextlib

import torch

DELAY_TARGET_MS = 100.0       # long against a call's host cost (tens of µs to a few ms after a warm-up)
DELAY_FLOOR_MS = 50.0         # a shorter measured delay fails the calibration: the cases must not pass vacuously

_delays = {}                  # device index -> (enqueue(), measured ms)


def _timed_ms(enqueue, device):
    """Milliseconds `enqueue()` occupies the current stream of `device`, by events."""
    with torch.cuda.device(device):
        t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize(device)
        t0.record()
        enqueue()
        t1.record()
        t1.synchronize()
        return t0.elapsed_time(t1)


def calibrate(device):
    """(enqueue, ms): `enqueue()` puts a device-side wait of about DELAY_TARGET_MS on the current stream of
    `device` (torch.cuda._sleep where torch has it, else a chain of element-wise ops on one large tensor),
    sized once per device and session from event timings; ms is the delay as measured afterwards."""
    device = torch.device(device)
    if device.index is None:
        device = torch.device("cuda", torch.cuda.current_device())
    if device.index in _delays:
        return _delays[device.index]
    if hasattr(torch.cuda, "_sleep"):
        def make(units):
            return lambda: torch.cuda._sleep(int(units))
        units = 1 << 20                                  # cycles of the device's counter
    else:
        big = torch.zeros(1 << 26, dtype=torch.float32, device=device)

        def make(units):
            def run():
                for _ in range(int(units)):
                    big.add_(1.0)
            return run
        units = 4                                        # passes over 256 MiB
    _timed_ms(make(units), device)                       # code objects
    ms = _timed_ms(make(units), device)
    for _ in range(8):                                   # a probe long enough to time: at least 5 ms
        if ms >= 5.0:
            break
        units *= 8
        ms = _timed_ms(make(units), device)
    units = max(1, int(units * DELAY_TARGET_MS / max(ms, 1e-3)))
    enqueue = make(units)
    ms = _timed_ms(enqueue, device)
    print(f"launch contract: delay on {device} calibrated to {ms:.1f} ms ({units} units)")
    assert ms >= DELAY_FLOOR_MS, f"the calibrated delay is {ms:.1f} ms, below {DELAY_FLOOR_MS} ms: the cases would prove nothing"
    _delays[device.index] = (enqueue, ms)
    return _delays[device.index]


def delay(stream):
    """Enqueue the calibrated device-side wait on `stream`."""
    enqueue, _ = calibrate(stream.device)
    with torch.cuda.stream(stream):
        enqueue()


@contextlib.contextmanager
def on_stream(stream):
    """`stream` is the current stream of its device; the current device stays the caller's (torch.cuda.stream
    alone would switch to the stream's device)."""
    cur = torch.cuda.current_device()
    with torch.cuda.stream(stream):
        with torch.cuda.device(cur):
            yield


def bits(t):
    """t as integers of its element size: NaNs, signed zeros and all compare as words."""
    if t.dtype.is_floating_point:
        return t.view({2: torch.int16, 4: torch.int32, 8: torch.int64}[t.element_size()])
    return t


def same_bits(a, b):
    return a.shape == b.shape and a.dtype == b.dtype and bool(torch.equal(bits(a), bits(b)))


def sentinel_(t):
    """Quiet NaN for floats, -1 for integers (all bits set for unsigned ones)."""
    if t.dtype.is_floating_point:
        return t.fill_(float("nan"))
    return t.fill_(255 if t.dtype == torch.uint8 else -1)


def decoy(t):
    """Valid, in-range, different data of t's shape: the rows rolled by one row and 17 samples."""
    if t.dim() >= 2:
        return torch.roll(t, (1, 17), dims=(0, -1)).contiguous()
    return torch.roll(t, 1).contiguous()


class Case:
    """One call under test.

    ins:      {name: tensor}, the true inputs (on `device`, complete before the protocol starts).
    make_outs: () -> {name: tensor}: every output, scratch and work buffer the call accepts, newly allocated.
    call:     (ins, outs, state) -> {name: tensor} or None: the engine call on the current stream; `state` is a
              dict that lives as long as one stream is used (a Workspace made under that stream); what the call
              allocates and returns itself comes back in the dict.
    zeroed:   the outs the call adds to (accumulators, reports): they start from 0, not from the sentinel.
    unchecked: the outs that are scratch or unordered sums: not compared.
    finish:   (state) -> None, run after the stream was waited for (a forward's Workspace.check() == 0).
    waits:    the reason, if the call waits on the host by contract (then `busy` is not asserted).
    """

    def __init__(self, device, ins, make_outs, call, zeroed=(), unchecked=(), finish=None, waits=None):
        self.device = torch.device(device)
        self.ins, self.make_outs, self.call = ins, make_outs, call
        self.zeroed, self.unchecked, self.finish, self.waits = set(zeroed), set(unchecked), finish, waits

    def init_(self, outs):
        for k, t in outs.items():
            t.zero_() if k in self.zeroed else sentinel_(t)

    def results(self, outs, extra):
        """What is compared: {name: tensor} of the checked outs and of what the call returned."""
        r = {k: t for k, t in outs.items() if k not in self.unchecked}
        for k, t in (extra or {}).items():
            assert k not in r
            r[k] = t
        return r


def reference(case):
    """Step 1: the call on the default stream of the case's device, on the true inputs: cloned results."""
    outs = case.make_outs()
    case.init_(outs)
    state = {}
    extra = case.call(case.ins, outs, state)
    torch.cuda.synchronize(case.device)
    if case.finish:
        case.finish(state)
    ref = {k: t.clone() for k, t in case.results(outs, extra).items()}
    torch.cuda.synchronize(case.device)
    for k, t in ref.items():                 # every output was written: none still holds the sentinel
        if t.dtype.is_floating_point:
            assert not torch.isnan(t).any(), f"reference {k} holds a NaN"
    return ref


def run_delayed(case, ref):
    """Steps 2 to 5 on a new side stream of the case's device.  Returns (busy, mismatches): whether the stream
    still had work when the call returned, and the names of the results that differ from `ref` in a bit."""
    dev = case.device
    staging = {k: decoy(t) for k, t in case.ins.items()}
    decoys = {k: t.clone() for k, t in staging.items()}
    outs = case.make_outs()
    calibrate(dev)
    torch.cuda.synchronize(dev)
    s = torch.cuda.Stream(device=dev)
    s.wait_stream(torch.cuda.current_stream(dev))
    state = {}
    with on_stream(s):                       # warm-up: code objects, LDS opt-ins, occupancy caches, allocator pools
        for k, t in staging.items():
            t.copy_(case.ins[k])
        case.init_(outs)
        case.call(staging, outs, state)
        s.synchronize()
        if case.finish:
            case.finish(state)
        for k, t in staging.items():
            t.copy_(decoys[k])
        case.init_(outs)
        for t in outs.values():              # whatever start the call expects, the run must make it itself
            sentinel_(t)
        s.synchronize()
    torch.cuda.synchronize(dev)
    with on_stream(s):
        delay(s)
        for k, t in staging.items():
            t.copy_(case.ins[k])
        case.init_(outs)
        extra = case.call(staging, outs, state)
        busy = not s.query()
    s.synchronize()
    if case.finish:
        case.finish(state)
    got = case.results(outs, extra)
    assert set(got) == set(ref), (sorted(got), sorted(ref))
    bad = [k for k in sorted(ref) if not same_bits(got[k], ref[k])]
    torch.cuda.synchronize(dev)
    return busy, bad
