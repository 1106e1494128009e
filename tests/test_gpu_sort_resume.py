"""GPU tests of the resumable SORT (pmce_sort_track_resume_f64 through ``tracker.sort_tracks(..., state=)``): a video fed in pieces
through one ``SortState`` gives the bits of the one launch over the whole video, whatever the pieces, and equal histories give equal
state bytes.  Everything is compared on the bit pattern with the device's own single launch (the yardstick the issue sets); ids, counts
and report order are compared with tests/tracker_ref.py as well.  The single launches are computed once per case and shared."""
import numpy as np
import pytest
import torch

import tracker_ref as TR
from test_gpu_tracker import DEV, T, bits
from tracker_ref import SCENE_SEEDS

pytestmark = pytest.mark.gpu

PIECES = {"ones": [1] * 40, "sevens": [7, 7, 7, 7, 7, 5], "empty-first": [33, 7], "empty-last": [34, 6]}
ARGS = {"defaults": dict(), "update_on_empty": dict(update_on_empty=True), "max_age3": dict(max_age=3), "max_tracks2": dict(max_tracks=2)}
STATE_DOUBLES = 56 * 64                  # include/pmce_hip.h: x [7][64], P [7][7][64], then the ints alive [64], id, tsu, streak, two counters
_whole = {}


def scene():
    p, c = TR.draw_scene(SCENE_SEEDS[0])
    return torch.from_numpy(p).to(DEV), torch.from_numpy(c).to(DEV)


def whole(name):
    """Today's single launch over the 40 frames and the restatement's discrete results, once per argument set."""
    if name not in _whole:
        p, c = scene()
        pn, cn = TR.draw_scene(SCENE_SEEDS[0])
        _whole[name] = (T().sort_tracks(p, c, **ARGS[name]), TR.sort_tracks(pn, cn, **{k: int(v) for k, v in ARGS[name].items()}))
    return _whole[name]


def feed(p, c, pieces, state, **kw):
    outs, at = [], 0
    for n in pieces:
        outs.append(T().sort_tracks(p[at:at + n], c[at:at + n], state=state, **kw))
        at += n
    assert at == p.shape[0]
    return [torch.cat([o[i] for o in outs]) for i in range(3)]


def same(got, want):
    return torch.equal(bits(got[0]), bits(want[0])) and torch.equal(got[1], want[1]) and torch.equal(got[2], want[2])


def alive_slots(state, seq=0):
    return state.buffer[seq, STATE_DOUBLES * 8:STATE_DOUBLES * 8 + 256].contiguous().view(torch.int32)


@pytest.mark.parametrize("args", list(ARGS))
@pytest.mark.parametrize("pieces", list(PIECES))
def test_pieces_equal_the_whole_launch(pieces, args):
    p, c = scene()
    assert int(c[33]) == 0 and sum(PIECES[pieces]) == 40
    want, (rt, rn, rs) = whole(args)
    state = T().SortState()
    got = feed(p, c, PIECES[pieces], state, **ARGS[args])
    assert same(got, want)
    assert np.array_equal(got[0][..., 4].cpu().numpy(), rt[..., 4]) and np.array_equal(got[1].cpu().numpy(), rn)     # ids in report order
    assert np.array_equal(got[2].cpu().numpy(), rs) and state.frames.tolist() == [40]
    if args == "max_tracks2":
        s = got[2].cpu().numpy()
        assert s[:33].any() and s[34:].any()                                          # the status bit on both sides of the borders
    if args == "max_age3":
        assert rt[..., 4].max() == 3 and whole("defaults")[1][0][..., 4].max() == 4   # person 2 coasts over frames 20, 21 and keeps its id


@pytest.mark.parametrize("args", list(ARGS))
def test_state_bytes_do_not_depend_on_the_pieces(args):
    p, c = scene()
    one = T().SortState()
    got = feed(p, c, [40], one, **ARGS[args])
    assert same(got, whole(args)[0])                                                  # a fresh zero state: today's output
    assert one.buffer.dtype == torch.uint8 and tuple(one.buffer.shape) == (1, T()._lib.load().pmce_sort_state_bytes())
    assert bool(one.buffer.any()) and 1 <= int(alive_slots(one).sum()) <= 3
    for pieces in PIECES.values():
        st = T().SortState()
        feed(p, c, pieces, st, **ARGS[args])
        assert torch.equal(st.buffer, one.buffer)
    dead = alive_slots(one) == 0                                                      # canonical bytes: a slot that is not alive is zeros
    rec = one.buffer[0, :STATE_DOUBLES * 8].contiguous().view(torch.float64).view(56, 64)
    assert not bool(rec[:, dead].any())


def test_clone_forks_a_state():
    p, c = scene()
    a = T().SortState()
    feed(p[:20], c[:20], [20], a)
    b = a.clone()
    ra = T().sort_tracks(p[20:], c[20:], state=a)
    assert b.frames.tolist() == [20] and a.frames.tolist() == [40] and not torch.equal(a.buffer, b.buffer)
    rb = T().sort_tracks(p[20:], c[20:], state=b)
    assert same(ra, rb) and torch.equal(a.buffer, b.buffer)
    assert same([torch.cat([x, y]) for x, y in zip(T().sort_tracks(p[:20], c[:20]), ra)], whole("defaults")[0])
    with pytest.raises(ValueError, match="max_age"):
        T().sort_tracks(p[:1], c[:1], state=b, max_age=2)


def test_two_sequences_and_a_sequence_without_frames():
    (p0, c0), (p1, c1) = (tuple(torch.from_numpy(x).to(DEV) for x in TR.draw_scene(s)) for s in SCENE_SEEDS)
    w0, w1 = whole("defaults")[0], T().sort_tracks(p1, c1)
    state = T().SortState(2)
    a = T().sort_tracks(p0, c0, seq_offsets=[0, 40, 40], state=state)
    assert same(a, w0) and not bool(state.buffer[1].any()) and bool(state.buffer[0].any())
    first = state.buffer[0].clone()
    b = T().sort_tracks(p1, c1, seq_offsets=[0, 0, 40], state=state)
    assert same(b, w1) and torch.equal(state.buffer[0], first) and state.frames.tolist() == [40, 40]
    # and interleaved in uneven pieces, both sequences in every launch
    st2, outs = T().SortState(2), []
    for (a0, b0), (a1, b1) in (((0, 33), (0, 1)), ((33, 34), (1, 1)), ((34, 40), (1, 40))):
        n0 = b0 - a0
        outs.append((T().sort_tracks(torch.cat([p0[a0:b0], p1[a1:b1]]), torch.cat([c0[a0:b0], c1[a1:b1]]),
                                     seq_offsets=[0, n0, n0 + b1 - a1], state=st2), n0))
    got0 = [torch.cat([o[i][:n0] for o, n0 in outs]) for i in range(3)]
    got1 = [torch.cat([o[i][n0:] for o, n0 in outs]) for i in range(3)]
    assert same(got0, w0) and same(got1, w1) and torch.equal(st2.buffer, state.buffer)
    with pytest.raises(ValueError, match="n_seq"):
        T().sort_tracks(p0, c0, state=st2)


def test_an_empty_call_leaves_the_state():
    p, c = scene()
    state = T().SortState()
    feed(p[:10], c[:10], [10], state)
    before = state.buffer.clone()
    t, n, s = T().sort_tracks(p[:0], c[:0], state=state)
    assert tuple(t.shape) == (0, 64, 5) and tuple(n.shape) == (0,) and tuple(s.shape) == (0,)
    assert torch.equal(state.buffer, before) and state.frames.tolist() == [10]
    assert same(feed(p[10:], c[10:], [30], state), [x[10:] for x in whole("defaults")[0]])


def test_crowd_of_64_trackers_across_every_border():
    """The wide crowd of tests/test_gpu_tracker_crowd.py (64 persons, max_age = 3: all 64 slots in use), one frame per launch: the
    state is carried over borders at which every slot is alive."""
    seed, persons, frames = TR.WIDE_CROWD
    pn, cn = TR.draw_crowd(seed, frames=frames, persons=persons)
    p, c = torch.from_numpy(pn).to(DEV), torch.from_numpy(cn).to(DEV)
    kw = TR.WIDE_PARAMS[0]
    want = T().sort_tracks(p, c, **kw)
    state, outs, alive = T().SortState(), [], []
    for f in range(frames):
        outs.append(T().sort_tracks(p[f:f + 1], c[f:f + 1], state=state, **kw))
        alive.append(alive_slots(state).sum())
    alive = torch.stack(alive).cpu().tolist()
    print("alive after each frame:", alive)
    assert max(alive[:-1]) == 64                                                      # a border with every slot alive
    assert same([torch.cat([o[i] for o in outs]) for i in range(3)], want) and not bool(want[2].any())
    one = T().SortState()
    T().sort_tracks(p, c, state=one, **kw)
    assert torch.equal(one.buffer, state.buffer)
