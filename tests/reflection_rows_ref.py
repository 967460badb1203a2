"""What tests/test_gpu_reflection_rows.py compares against: the reference's own FFT-domain formula (waveforms/
distortion.py:188-223), restated in NumPy and applied row by row, and the seeded rows and term lists of its cases."""
import numpy as np


def reflection_filter(f, A, tau):
    """reference distortion.py:188-205"""
    return (1 - A) / (1 - A * np.exp(-2j * np.pi * f * tau))


def transfer(terms, f):
    """the product of a row's terms at the frequencies f"""
    H = np.ones(len(f), dtype=np.complex128)
    for term in terms:
        if term[0] == 'reflect':
            H = H * reflection_filter(f, term[1], term[2])
        elif term[0] == 'correct':
            H = H / reflection_filter(f, term[1], term[2])
        else:
            H = H * np.exp(-2j * np.pi * f * term[1])
    return H


def ref_row(x, terms, fs):
    """ifft(fft(x) * H(fftfreq)).real -- reflection / correct_reflection of the reference, any product of terms"""
    return np.fft.ifft(np.fft.fft(x) * transfer(terms, np.fft.fftfreq(len(x), 1 / fs))).real


def ref_rows(x, terms_rows, fs):
    return np.stack([ref_row(row, terms, fs) for row, terms in zip(x, terms_rows)])


def rows_input(n, rows, seed):
    rng = np.random.default_rng(seed)
    return np.cumsum(rng.normal(size=(rows, n)), axis=1) / 30 + 0.01 * rng.normal(size=(rows, n))


def random_term(rng, kind=None):
    """|A| <= 0.3, tau <= 200 ns (a delay of either sign)"""
    kind = kind or ('reflect', 'correct', 'delay')[int(rng.integers(3))]
    if kind == 'delay':
        return ('delay', float(rng.uniform(-200e-9, 200e-9)))
    return (kind, float(rng.uniform(-0.3, 0.3)), float(rng.uniform(0, 200e-9)))


def rows_terms(rows, seed):
    """row r carries r mod 4 terms: a batch of 5 holds two 0-term rows, a single reflection, and products of two and
    three terms of mixed kinds"""
    rng = np.random.default_rng(seed)
    return [[random_term(rng, 'reflect' if r % 4 == 1 else None) for _ in range(r % 4)] for r in range(rows)]
