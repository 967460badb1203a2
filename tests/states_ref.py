"""The referee of the state discriminator (utils.StateDiscriminator, csrc/wfk_states.hip), in NumPy on the host.

points (S, nf) complex128, centres (nf, K) complex128 (NaN pads a tone with fewer states).  Per shot, tone and state

    dr = re(p) - re(c),  di = im(p) - im(c),  d2 = dr * dr + di * di        (float64, every operation rounded on its own)

and the label is the NumPy line `d2 = where(isfinite(d2), d2, inf); argmin(d2, -1)`, with 255 where the minimum is inf:
argmin takes the first minimum (ties go to the lowest state), a NaN or infinite distance never wins.  From the labels:
the packed word of a shot (tone j in bits [j b, (j + 1) b), -1 when a tone is invalid), the counts per step
(steps, nf, K + 1) and the joint histogram of the words (steps, 2^(nf b) + 1); shot s of a block that `first` shots
precede belongs to step (first + s) % steps.  `brute_force` is the same by Python loops.  A plain module like avg_ref.py."""
import numpy as np

INVALID = 255


def bits_of(K):
    return 1 if K <= 2 else 2 if K <= 4 else 3


def distances(points, centres):
    """(S, nf, K) float64"""
    points, centres = np.asarray(points, dtype=np.complex128), np.asarray(centres, dtype=np.complex128)
    with np.errstate(all='ignore'):
        dr = points.real[:, :, None] - centres.real[None]
        di = points.imag[:, :, None] - centres.imag[None]
        return dr * dr + di * di


def labels_ref(points, centres):
    """(S, nf) uint8"""
    d2 = distances(points, centres)
    d2 = np.where(np.isfinite(d2), d2, np.inf)
    labels = np.argmin(d2, -1).astype(np.uint8)
    labels[np.min(d2, -1) == np.inf] = INVALID
    return labels


def words_ref(labels, K):
    """(S,) int64; nf * bits_of(K) <= 62"""
    labels = np.asarray(labels)
    S, nf = labels.shape
    b = bits_of(K)
    assert nf * b <= 62
    words = np.zeros(S, dtype=np.int64)
    for j in range(nf):
        words |= labels[:, j].astype(np.int64) << (j * b)
    words[(labels == INVALID).any(axis=1)] = -1
    return words


def steps_of_block(shots, first, steps):
    """(shots,) int64: the step of every shot of a block (`first` may be any Python int)"""
    return (int(first) % int(steps) + np.arange(shots, dtype=np.int64)) % int(steps)


def counts_ref(labels, K, steps, first=0, old=None):
    """(steps, nf, K + 1) int64; old: the accumulate base (None: overwrite)"""
    labels = np.asarray(labels)
    S, nf = labels.shape
    column = np.where(labels == INVALID, K, labels).astype(np.int64)
    index = (steps_of_block(S, first, steps)[:, None] * nf + np.arange(nf)[None]) * (K + 1) + column
    counts = np.bincount(index.reshape(-1), minlength=steps * nf * (K + 1)).astype(np.int64).reshape(steps, nf, K + 1)
    return counts if old is None else np.asarray(old, dtype=np.int64) + counts


def joint_ref(words, n_bits, steps, first=0, old=None):
    """(steps, 2^n_bits + 1) int64: bin w the shots whose word is w, the last bin those with word -1"""
    words = np.asarray(words, dtype=np.int64)
    bins = 2 ** n_bits + 1
    which = np.where(words < 0, bins - 1, words)
    index = steps_of_block(len(words), first, steps) * bins + which
    joint = np.bincount(index, minlength=steps * bins).astype(np.int64).reshape(steps, bins)
    return joint if old is None else np.asarray(old, dtype=np.int64) + joint


def brute_force(points, centres, steps, first=0):
    """-> (labels, words, counts, joint) by loops over shots, tones and states in Python floats and ints; joint is
    None where nf * bits > 16, words where it is > 62"""
    points, centres = np.asarray(points, dtype=np.complex128), np.asarray(centres, dtype=np.complex128)
    S, nf = points.shape
    K = centres.shape[1]
    b = bits_of(K)
    inf = float('inf')
    labels = np.zeros((S, nf), dtype=np.uint8)
    words = np.zeros(S, dtype=np.int64) if nf * b <= 62 else None
    counts = np.zeros((steps, nf, K + 1), dtype=np.int64)
    joint = np.zeros((steps, 2 ** (nf * b) + 1), dtype=np.int64) if nf * b <= 16 else None
    for s in range(S):
        g = (first + s) % steps
        word, bad = 0, False
        for j in range(nf):
            best, winner = inf, None
            for k in range(K):
                dr = float(points[s, j].real) - float(centres[j, k].real)
                di = float(points[s, j].imag) - float(centres[j, k].imag)
                try:
                    d2 = dr * dr + di * di
                except OverflowError:
                    d2 = inf
                if d2 < best:
                    best, winner = d2, k
            if winner is None:
                labels[s, j], bad = INVALID, True
                counts[g, j, K] += 1
            else:
                labels[s, j] = winner
                word |= winner << (j * b)
                counts[g, j, winner] += 1
        if words is not None:
            words[s] = -1 if bad else word
        if joint is not None:
            joint[g, -1 if bad else word] += 1
    return labels, words, counts, joint
