"""The hand-off object of the graph runner (eagcn_amd/graph.py: FlagHandoff / EventHandoff), driven on the CPU with a fake library
and fake streams and events that record every call.  The expected sequences are written out by hand from the protocol:

Flag form (S = forwards executed so far): a preparation with `overlap` makes the side stream wait for the start counter to reach S
when S >= 2 (eagcn_stream_wait_counter(start_word, S & 0xFFFFFFFF, side)), none without `overlap`; behind the preparation,
eagcn_stream_signal_flag(ready + 4 * slot) on the stream that prepared; both Model structs carry wait_flag = ready + 4 * slot and
start_signal = start_word; reset = synchronise, zero both flags, start_word = S as an int32, synchronise.

Event form: every preparation records an event on the main stream (that position is what the NEXT overlapped preparation has to
wait for, so it is recorded without `overlap` too); with `overlap` the side stream waits for the event of the PREVIOUS preparation,
if any, and behind the preparation the main stream waits for an event recorded on the side stream; without `overlap` nothing else
is recorded and nothing is waited for; the Model structs carry no hand-off words; reset does nothing.

Both: an unfused forward with `overlap` records `fwd_done` on the main stream and the next preparation's side stream waits for it;
a fused step clears it.  No torch device call is made."""
import types

import pytest

from eagcn_amd.graph import EventHandoff, FlagHandoff

READY, START = 0x7000, 0x7100
MAIN, SIDE = 11, 22


class Log(list):
    pass


class FakeStream:
    def __init__(self, log, name, handle):
        self.log, self.name, self.cuda_stream = log, name, handle

    def wait_event(self, ev):
        self.log.append(('wait_event', self.name, ev.n))


class FakeEvent:
    def __init__(self, log):
        self.log, self.n = log, log.events
        log.events += 1

    def record(self, stream):
        self.log.append(('record', self.n, stream.name))


class FakeLib:
    def __init__(self, log):
        self.log = log

    def eagcn_stream_wait_counter(self, word, value, stream):
        self.log.append(('wait_counter', word, value, stream))
        return 0

    def eagcn_stream_signal_flag(self, word, stream):
        self.log.append(('signal_flag', word, stream))
        return 0


class FakeWords:
    def __init__(self, log):
        self.log = log

    def synchronize(self):
        self.log.append('synchronize')

    def zero_ready(self):
        self.log.append('zero_ready')

    def set_start(self, v):
        self.log.append(('set_start', v))


def make(form):
    log = Log()
    log.events = 0
    new_event = lambda: FakeEvent(log)                                   # noqa: E731
    h = FlagHandoff(new_event, FakeLib(log), READY, START, FakeWords(log)) if form == 'flag' else EventHandoff(new_event)
    return h, log, FakeStream(log, 'main', MAIN), FakeStream(log, 'side', SIDE)


def drive(h, log, main, side, overlap):
    """Steps 0 .. 5: prepare (begin, ready), then one executed forward; one more forward counted before step 3 (attributions)."""
    per_step = []
    for k in range(6):
        if k == 3:
            h.started()
        del log[:]
        prep = side if overlap else main
        h.begin(main, prep, overlap)
        log.append('PREPARE')
        h.ready(k % 2, main, prep, overlap)
        h.started()
        per_step.append(list(log))
    return per_step


@pytest.mark.parametrize('overlap', [False, True], ids=['plain', 'overlap'])
def test_flag_form_sequence(overlap):
    h, log, main, side = make('flag')
    got = drive(h, log, main, side, overlap)
    stream = SIDE if overlap else MAIN
    forwards = [0, 1, 2, 4, 5, 6]                     # S in front of step k (the extra forward before step 3)
    want = []
    for k, S in enumerate(forwards):
        seq = []
        if overlap and S >= 2:
            seq.append(('wait_counter', START, S, SIDE))
        seq += ['PREPARE', ('signal_flag', READY + 4 * (k % 2), stream)]
        want.append(seq)
    assert got == want
    assert want[1] == ['PREPARE', ('signal_flag', READY + 4, stream)]                      # (spelled out: no wait while S < 2)
    if overlap:
        assert want[3] == [('wait_counter', START, 4, SIDE), 'PREPARE', ('signal_flag', READY + 4, SIDE)]
    assert h.starts == 7


@pytest.mark.parametrize('overlap', [False, True], ids=['plain', 'overlap'])
def test_event_form_sequence(overlap):
    h, log, main, side = make('event')
    got = drive(h, log, main, side, overlap)
    want, n, prev = [], 0, None
    for k in range(6):
        seq = [('record', n, 'main')]                 # this preparation's main-stream position
        mine, n = n, n + 1
        if overlap and prev is not None:
            seq.append(('wait_event', 'side', prev))
        seq.append('PREPARE')
        if overlap:
            seq += [('record', n, 'side'), ('wait_event', 'main', n)]
            n += 1
        prev = mine
        want.append(seq)
    assert got == want
    if overlap:
        assert want[0] == [('record', 0, 'main'), 'PREPARE', ('record', 1, 'side'), ('wait_event', 'main', 1)]
        assert want[2] == [('record', 4, 'main'), ('wait_event', 'side', 2), 'PREPARE', ('record', 5, 'side'), ('wait_event', 'main', 5)]
    else:
        assert want[2] == [('record', 2, 'main'), 'PREPARE']
    assert h.starts == 7                              # counted in this form too (one rule for both)


@pytest.mark.parametrize('form', ['flag', 'event'])
def test_model_words(form):
    h = make(form)[0]
    for slot in (0, 1):
        m = types.SimpleNamespace(wait_flag=123, start_signal=456)
        h.wire(m, slot)
        assert (m.wait_flag, m.start_signal) == ((READY + 4 * slot, START) if form == 'flag' else (None, None))
    m = types.SimpleNamespace(wait_flag=123, start_signal=456)
    h.wire(m)                                         # the later forwards of an attribution graph: no hand-off
    assert (m.wait_flag, m.start_signal) == (None, None)


@pytest.mark.parametrize('S, word', [(3, 3), (2 ** 31 + 5, 2 ** 31 + 5 - 2 ** 32)])
def test_reset_words(S, word):
    h, log, main, side = make('flag')
    h.starts = S
    h.reset()
    assert log == ['synchronize', 'zero_ready', ('set_start', word), 'synchronize']
    assert -2 ** 31 <= word < 2 ** 31 and word % 2 ** 32 == S % 2 ** 32
    del log[:]
    h.begin(main, side, True)                         # ... and the count the side stream then waits for is the uint32 of S
    assert log == [('wait_counter', START, S & 0xFFFFFFFF, SIDE)]
    e, elog, _, _ = make('event')
    e.starts = S
    e.reset()
    assert elog == []


@pytest.mark.parametrize('form', ['flag', 'event'])
def test_forward_done_holds_the_next_preparation_back(form):
    h, log, main, side = make(form)
    h.begin(main, side, True)
    h.ready(0, main, side, True)
    h.started()
    h.forward_done(main)                              # unfused forward with overlap
    done = log.events - 1
    assert log[-1] == ('record', done, 'main')
    del log[:]
    h.begin(main, side, True)
    assert log[-1] == ('wait_event', 'side', done)    # behind the slot-free wait, if any
    assert [c for c in log if c[0] == 'wait_event' and c[2] == done] == [('wait_event', 'side', done)]
    h.ready(1, main, side, True)
    h.started()
    del log[:]
    h.begin(main, main, False)                        # without overlap the preparation is on the main stream: no wait
    assert not [c for c in log if c[0] == 'wait_event']
    h.ready(0, main, main, False)
    h.started()
    h.step_done()                                     # a fused step clears it
    del log[:]
    h.begin(main, side, True)
    assert not [c for c in log if c[0] == 'wait_event' and c[2] == done]
