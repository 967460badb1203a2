"""The referee of the trace averager (utils.TraceAverager, csrc/wfk_avg.hip), in NumPy on the host.

A block of S traces, `first` shots of the run before it, G steps:

    shot s of the block belongs to step (first + s) % G

sum[g] is the sum of the block's traces of step g, sumsq[g] that of their squares; accumulate adds them to `old` and
leaves a step without a shot in the block as it was, else a step without a shot is 0.  Integer traces are summed in
int64 (exact: |code| <= 2^15, so 2^33 shots fit; squares in int64 too), float traces in np.longdouble after widening to
float64, which is what the device's fp64 results are held against.  A plain module like curve_rows_ref.py."""
import numpy as np


def step_of(s, first, steps):
    return (first + s) % steps


def steps_of_block(shots, first, steps):
    """(shots,) the step of every shot of a block (Python ints: `first` may be anything)"""
    return np.array([step_of(s, int(first), int(steps)) for s in range(shots)], dtype=np.int64)


def counts_ref(shots, first, steps):
    return np.bincount(steps_of_block(shots, first, steps), minlength=steps).astype(np.int64)


def wide(x):
    """what the sums are formed of: int64 for codes, longdouble (through float64) for floats"""
    x = np.asarray(x)
    return x.astype(np.int64) if x.dtype.kind == 'i' else x.astype(np.float64).astype(np.longdouble)


def sums_ref(x, steps, first=0, old_sum=None, old_sumsq=None):
    """x (S, N) -> (sum, sumsq), each (steps, N) int64 or longdouble; old_*: the accumulate base (None: overwrite)"""
    w = wide(x)
    S, N = w.shape
    # the shots laid out cycle by cycle: shot s sits in cycle (first % G + s) // G at its step; the holes are zeros
    cycle, step = np.divmod(int(first) % int(steps) + np.arange(S), int(steps))
    assert np.array_equal(step, steps_of_block(S, first, steps))
    present = np.bincount(step, minlength=steps) > 0
    out = []
    for terms, old in ((w, old_sum), (w * w, old_sumsq)):
        laid = np.zeros((int(cycle[-1]) + 1 if S else 0, steps, N), dtype=w.dtype)
        laid[cycle, step] = terms
        block = laid.sum(axis=0)
        if old is None:
            out.append(block)
        else:
            acc = np.array(old).astype(w.dtype)
            acc[present] = acc[present] + block[present]
            out.append(acc)
    return out[0], out[1]


def brute_force(x, steps, first=0):
    """the same by a double loop over shots and columns, in Python ints / longdouble scalars"""
    x = np.asarray(x)
    integer = x.dtype.kind == 'i'
    zero = 0 if integer else np.longdouble(0)
    S, N = x.shape
    total = [[zero] * N for _ in range(steps)]
    total_sq = [[zero] * N for _ in range(steps)]
    for s in range(S):
        g = (first + s) % steps
        for c in range(N):
            v = int(x[s, c]) if integer else np.longdouble(np.float64(x[s, c]))
            total[g][c] += v
            total_sq[g][c] += v * v
    dtype = np.int64 if integer else np.longdouble
    return np.array(total, dtype=dtype).reshape(steps, N), np.array(total_sq, dtype=dtype).reshape(steps, N)


def bounds(x, steps, first=0, old_sum=None, old_sumsq=None):
    """the float bounds per (step, column), with m = the block's shots of the step (+ 1 with an accumulate base):
    |sum - exact| <= (m - 1) 2^-52 SUM|terms| and |sumsq - exact| <= m 2^-52 SUM terms^2 -> (bound_sum, bound_sumsq),
    longdouble.  Recursive summation at unit roundoff 2^-53, doubled for its higher-order terms and one rounding per
    square."""
    w = wide(x)
    step = steps_of_block(len(w), first, steps)
    m = np.bincount(step, minlength=steps).astype(np.longdouble)[:, None]
    mag, _ = sums_ref(np.abs(np.asarray(x, dtype=np.float64)), steps, first)
    _, sq = sums_ref(x, steps, first)
    if old_sum is not None:
        m = m + 1
        mag = mag + np.abs(np.asarray(old_sum).astype(np.longdouble))
        if old_sumsq is not None:
            sq = sq + np.abs(np.asarray(old_sumsq).astype(np.longdouble))
    eps = np.longdouble(2.0) ** -52
    return np.maximum(m - 1, 0) * eps * mag, m * eps * sq
