"""The stream contract of include/geoadv.h, as one deterministic protocol (tests/test_gpu_stream_order.py runs every
stream-taking entry point through it; DESIGN.md, 'The stream contract').

The header promises that a call only ENQUEUES on the stream it is given.  A launch, memset or copy that forgets the stream
lands on the null stream; a suite that runs on the null stream itself cannot see that, and neither can a second run of the same
input on an idle side stream: every intermediate buffer already holds the right values and nothing is queued ahead of the
stray launch.  `check` makes the mistake visible:

  1. WANT     the entry point on the default stream on input B, synchronised; the bytes of every output and of the state it changes
  2. REPEAT   the same again (from a twin handle where a call changes state): the same bytes
  3. STALE    every buffer the delayed call reads before it writes is made to hold values derived from ANOTHER well-formed input
              A: the same outputs and caller-owned scratch after a call on A; a handle's own scratch after a call on A; for
              trainers and the attack a fresh twin handle (a zero-filled arena) whose input buffer holds A.  Never a byte
              pattern: a launch that really is off its stream then reads wrong numbers, never wild indices
  4. DELAYED  on a side stream S: a delay; a device-to-device copy of B into the input buffers; an event; the entry point.
              The event must not have completed when the call is made, nor -- for an entry point that promises not to
              synchronise the host -- when it returns.  Then S is synchronised and outputs and state must equal step 1 byte for
              byte.
Everything the call queues on S waits behind the delay; whatever it sends elsewhere runs at once, on A-derived or zero data,
and either leaves a wrong value behind or feeds one to the launches that follow it on S.  There are no retries: a mismatch is a
failure.

THE DELAY is torch-only work on S: torch.cuda._sleep (a chain of large matmuls if a build lacks it), its cycles calibrated
against events once per session.  It is sized once per session, from the host-side enqueue time of the slowest covered call
(the `probe` the test module hands to `session_delay`): ten times that time, at least 50 ms, at most 500 ms.
MEASURED on the MI355X (host time of the warm call of step 2, ms): see ENQUEUE_NOTE below, which the test module's report
test prints afresh (-s).  Both event queries of step 4 are assertions, so a delay that was too short fails a case; it never
lets one pass vacuously.
"""
import time

import numpy as np
import torch

MIN_DELAY_MS, MAX_DELAY_MS, MARGIN = 50.0, 500.0, 10.0
ENQUEUE_NOTE = ("slowest host-side enqueues measured on the MI355X, ms: cls_trainer_step 5.6 on the first twin handle of a "
                "session (0.98 on later ones), fold_trainer_step 0.63, atlas_trainer_step 0.55, trainer_export 0.54, the "
                "AE trainer's phases 0.44, the attack sequence (set_inputs, init_pert, run(3), get_best, peek, test readers) "
                "0.40, every stateless operator below 0.4; the probe takes the largest of the first three, so the delay "
                "chosen is 10 x 5.6 = 56 ms where the first-handle cost shows and the 50 ms floor otherwise")
ENQUEUE_MS = {}             # case name -> host milliseconds of the warm call of step 2 (the report test prints it)


class Delay:
    """delay() queues `ms` milliseconds of torch-only work on the current stream."""

    def __init__(self):
        self.ms = MIN_DELAY_MS
        self.probe_ms = None
        self._sleep = getattr(torch.cuda, "_sleep", None)
        if self._sleep is not None:
            self._unit, cycles = "cycles", 20_000_000
            self._sleep(1_000_000)                               # the sleep kernel's first launch loads its code object
            took = self._time(lambda: self._sleep(cycles))
            self._per_ms = cycles / max(took, 1e-3)
        else:
            self._unit = "matmuls"
            self._a = torch.randn((4096, 4096), device="cuda:0")
            self._chain(2)
            self._per_ms = 16 / max(self._time(lambda: self._chain(16)), 1e-3)

    def _chain(self, count):
        a = self._a
        for _ in range(int(count)):
            a = (a @ self._a) * (1.0 / 4096.0)
        return a

    @staticmethod
    def _time(work):
        torch.cuda.synchronize()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        work()
        e1.record()
        e1.synchronize()
        return e0.elapsed_time(e1)

    def size(self, enqueue_ms):
        self.probe_ms = float(enqueue_ms)
        self.ms = min(MAX_DELAY_MS, max(MIN_DELAY_MS, MARGIN * self.probe_ms))

    def __call__(self):
        amount = max(1, int(self.ms * self._per_ms))
        if self._unit == "cycles":
            self._sleep(amount)
        else:
            self._chain(amount)


_SESSION = {}


def session_delay(probe=None):
    """The session's Delay, built and sized on first use.  probe() makes the slowest covered call once, warm, on the default
    stream and returns its host-side enqueue time in milliseconds."""
    if "delay" not in _SESSION:
        _SESSION["delay"] = Delay()
    d = _SESSION["delay"]
    if probe is not None and d.probe_ms is None:             # (a module without a probe may have built it first: the floor)
        d.size(probe())
    return d


class Rig:
    """One entry point (or one sequence of them) on fixed buffers.
    feeds   [(buffer, A, B)]: device tensors of one shape and dtype; `buffer` is what the call reads, A and B two different
            well-formed inputs
    call    () -> a sequence of device tensors, numpy arrays and host values: the outputs.  It makes the library calls with the
            CURRENT torch stream's handle and returns without waiting for the device
    state   () -> device tensors viewing the handle state the call changes (compared like outputs)
    keep    whatever must stay alive as long as the rig (handles, workspaces)"""

    def __init__(self, feeds, call, state=None, keep=None):
        self.feeds, self.call, self.state, self.keep = list(feeds), call, state or (lambda: []), keep
        for buf, a, b in self.feeds:
            assert buf.shape == a.shape == b.shape and buf.dtype == a.dtype == b.dtype, "feeds must agree in shape and type"
            assert not _same(a, b), "inputs A and B of a feed must differ"

    def load(self, which):
        for buf, a, b in self.feeds:
            buf.copy_(a if which == "A" else b)

    def result(self, out):
        return _snapshot(list(out) + list(self.state()))


def _snapshot(values):
    out = []
    for v in values:
        if isinstance(v, torch.Tensor):
            out.append(v.detach().clone())
        elif isinstance(v, np.ndarray):
            out.append(v.copy())
        else:
            out.append(v)
    return out


def _same(a, b):
    if isinstance(a, torch.Tensor):
        if not isinstance(b, torch.Tensor) or a.dtype != b.dtype or a.shape != b.shape:
            return False
        return torch.equal(a.contiguous().reshape(-1).view(torch.uint8), b.contiguous().reshape(-1).view(torch.uint8))
    if isinstance(a, np.ndarray):
        return isinstance(b, np.ndarray) and a.dtype == b.dtype and a.shape == b.shape and a.tobytes() == b.tobytes()
    return type(a) is type(b) and a == b


def differences(got, want):
    """Indices of the outputs / state entries whose bytes differ."""
    assert len(got) == len(want), "the call returned %d values, then %d" % (len(want), len(got))
    return [i for i, (g, w) in enumerate(zip(got, want)) if not _same(g, w)]


def check(name, build, delay, stateful=False, blocks=None):
    """The protocol for one case.  build() -> Rig; it is called once for a stateless entry point and once per step for a
    stateful one (twins from the same initial state).  blocks: None for an entry point that must not synchronise the host,
    else the header sentence that says it does (it is then held to the ordering alone)."""
    assert blocks is None or (isinstance(blocks, str) and blocks.strip()), "an excuse is a quoted header sentence"
    dev = torch.device("cuda:0")
    assert torch.cuda.current_stream(dev).cuda_stream == 0, "the protocol starts on the default (null) stream"
    # 1. want
    rig = build()
    rig.load("B")
    out = rig.call()
    torch.cuda.synchronize()
    want = rig.result(out)
    assert want, "%s: nothing to compare" % name
    # 2. repeat
    again = build() if stateful else rig
    again.load("B")
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    out = again.call()
    ENQUEUE_MS[name] = (time.perf_counter() - t0) * 1e3
    torch.cuda.synchronize()
    diff = differences(again.result(out), want)
    assert not diff, "%s: two calls on the same input differ in outputs %s (not byte-repeatable)" % (name, diff)
    # 3. stale but well-formed
    late = build() if stateful else rig
    late.load("A")
    if not stateful:
        late.call()
    torch.cuda.synchronize()
    # 4. the delayed call
    side = torch.cuda.Stream(dev)
    e_delay = torch.cuda.Event()
    with torch.cuda.stream(side):
        delay()
        late.load("B")
        e_delay.record(side)
        pending_before = not e_delay.query()
        out = late.call()
        pending_after = not e_delay.query()
    assert pending_before, ("%s: the delay of %.0f ms had run out before the call was made -- the case would prove nothing"
                            % (name, delay.ms))
    if blocks is None:
        assert pending_after, ("%s: the delay (%.0f ms) had completed when the call returned: the call blocked the host on its "
                               "stream, and the header has no sentence that says so" % (name, delay.ms))
    side.synchronize()
    torch.cuda.synchronize()
    diff = differences(late.result(out), want)
    assert not diff, ("%s: behind a delay on a side stream the outputs / state %s differ from the default-stream run: some launch, "
                      "memset or copy of the call did not go to the stream it was given" % (name, diff))


def check_call(name, fn, inputs_a, inputs_b, keep=None, blocks=None):
    """The protocol for a stateless call fn(*buffers) -> outputs (a wrapper method of a model handle, say) on two sets of
    device tensors of equal shapes, with the session's delay."""
    feeds = [(a.clone(), a, b) for a, b in zip(inputs_a, inputs_b)]
    rig = Rig(feeds, lambda: fn(*[f[0] for f in feeds]), keep=keep)
    check(name, lambda: rig, session_delay(), blocks=blocks)


def control(delay, on_side_stream):
    """The protocol with a torch multiply in place of the entry point: x holds A; S gets the delay and then x.copy_(B); y = 2 x
    is computed on the default stream without waiting (on_side_stream False) or on S (True).  -> (y, A, B, the delay was still
    pending after the multiply was queued)."""
    dev = torch.device("cuda:0")
    g = torch.Generator().manual_seed(11)
    a = torch.rand((1 << 16,), generator=g).to(dev)
    b = torch.rand((1 << 16,), generator=g).to(dev)
    x = a.clone()
    y = torch.zeros_like(x)
    torch.cuda.synchronize()
    side = torch.cuda.Stream(dev)
    e_delay = torch.cuda.Event()
    with torch.cuda.stream(side):
        delay()
        x.copy_(b)
        e_delay.record(side)
        if on_side_stream:
            torch.mul(x, 2.0, out=y)
    if not on_side_stream:
        torch.mul(x, 2.0, out=y)
        torch.cuda.current_stream(dev).synchronize()          # the default stream only: S is still behind its delay
    pending = not e_delay.query()
    side.synchronize()
    torch.cuda.synchronize()
    return y, a, b, pending
