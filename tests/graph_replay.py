"""One apply captured into a graph and replayed on other data (include/wfk.h, "Graph capture").

An apply that "allocates nothing and does not synchronise" may be captured with `torch.cuda.graph` and replayed once per
shot: every `apply_torch` / `launch_torch` launches on torch's current stream, so the capture takes it as it is.  A
capture freezes what the apply was GIVEN -- pointers, strides, scalars -- and replays what it LAUNCHED; anything a launch
took from the host at that moment (a counter, say) is frozen with it.  `replay` is the one way the suite does this:

    got = replay(run, statics, feeds, outputs)      # got[k][j]: output j after the replay on feed k, a host array

`run()` applies the stage from the tensors of `statics` into those of `outputs` (device tensors, possibly windows of
wider ones; an in-place stage lists the same tensor on both sides).  A feed is one host array (or tensor) per static.
Capture is on ONE stream: no fork, no join, no second stream inside it.  At most three replays.  The helper sets no
environment variable.  A plain module like row_windows.py.

`eager` is the same load-run-read on the current stream without a graph: what a twin plan gives for the same feed."""
import numpy as np

from row_windows import _SENTINEL, _int_view

MAX_REPLAYS = 3
_SENTINEL_1 = 0xAA - 256                    # one-byte outputs (marker bytes are 0 or 1); int8 view


def _bits(t):
    import torch
    return t.view(torch.int8) if t.element_size() == 1 else _int_view(t)


def _sentinel_of(itemsize):
    return _SENTINEL_1 if itemsize == 1 else _SENTINEL[itemsize]


def _load(statics, feed, outputs):
    """the outputs filled with the sentinel's bits (a NaN with a payload for floats, a fixed code for integers), THEN
    the feed copied into the statics: a tensor that is both (in place, an accumulate base) ends up holding its feed"""
    import torch
    assert len(feed) == len(statics), (len(feed), len(statics))
    for o in outputs:
        b = _bits(o)
        b.fill_(_sentinel_of(b.element_size()))
    for s, f in zip(statics, feed):
        src = f if isinstance(f, torch.Tensor) else torch.from_numpy(np.array(np.broadcast_to(np.asarray(f), tuple(s.shape))))
        assert src.dtype == s.dtype and tuple(src.shape) == tuple(s.shape), (src.dtype, s.dtype, src.shape, s.shape)
        s.copy_(src)


def _read(outputs):
    import torch
    torch.cuda.synchronize()
    return [o.contiguous().cpu().numpy() for o in outputs]


def replay(run, statics, feeds, outputs):
    """warm `run()` up once eagerly on a side stream (on the first feed), capture ONE call of it, then for each feed:
    load, replay, synchronise, read.  -> one list of host arrays (one per output) per feed.  A capture the runtime
    refuses (an allocation, a blocking copy or a synchronisation inside `run`) raises out of here."""
    import torch
    assert 1 <= len(feeds) <= MAX_REPLAYS, len(feeds)
    _load(statics, feeds[0], outputs)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        run()
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        run()
    got = []
    for feed in feeds:
        _load(statics, feed, outputs)
        graph.replay()
        got.append(_read(outputs))
    del graph
    return got


def eager(run, statics, feed, outputs):
    """load, one eager `run()` on the current stream, synchronise, read -> a list of host arrays, one per output"""
    _load(statics, feed, outputs)
    run()
    return _read(outputs)


def sentinels_left(a):
    """how many elements of the host array `a` still hold the sentinel's bits (complex: in either component)"""
    a = np.ascontiguousarray(a)
    if a.dtype.kind == 'c':
        a = a.view(a.real.dtype)
    size = a.dtype.itemsize
    view = a.view({1: np.int8, 2: np.int16, 4: np.int32, 8: np.int64}[size])
    return int(np.count_nonzero(view == _sentinel_of(size)))
