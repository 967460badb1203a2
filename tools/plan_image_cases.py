#!/usr/bin/env python3
"""Writes the case directory that tools/plan_image.cpp compiles (tools/plan_image.sh runs both).

    python tools/plan_image_cases.py OUT_DIR [--random N]

One file per case: the wfk_program counts and arrays exactly as `_flatten.flatten` lays them out, the grid or
the time list, the request (keep_mixed_short, no_short_fmul, tlist_ns), the environment to set for the compile,
and for wfk_compile_blocks the thread count.  A case may name a BASELINE: it is then a witness, the same plan
with one switch thrown, and the image program fails if the two images are equal.

The list: the sampler plans of tests/test_kernel_names.py with their environments; cases.CASES, AWG_CASES at three
lengths, far_from_origin_case, the fine-grid list and the malformed programs of tools/sanitize/run_sanitized.py
and N random scripts, every one as a grid and as a jittered time list; a witness per request switch and per
environment switch of the compiler's table; plans for every retry of the ladder; wfk_compile_geom at the two
chain geometries; wfk_compile_blocks on 2, 3 and 4 threads; plans that reach the branches of the piece loop which
none of these takes (`reach.*`: found with the coverage build of tools/plan_image.sh); the three timing workloads."""
import argparse
import os
import struct
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, 'tests')]

import cases  # noqa: E402
import test_kernel_names as tkn  # noqa: E402
import waveforms_amd as wf  # noqa: E402
from waveforms_amd import _flatten, workloads as wl  # noqa: E402

ARRAYS = ['ch_member_off', 'ch_offset', 'ch_tshift', 'ch_clip_lo', 'ch_clip_hi', 'mb_piece_off', 'pc_bound',
          'pc_term_off', 'tm_amp_re', 'tm_amp_im', 'tm_factor_off', 'fc_type', 'fc_power', 'fc_shift', 'fc_arg_off',
          'pool']
DTYPES = dict(ch_member_off=np.int32, mb_piece_off=np.int32, pc_term_off=np.int32, tm_factor_off=np.int32,
              fc_type=np.int32, fc_arg_off=np.int64)
COMPILE, GEOM, BLOCKS = 0, 1, 2
INTERLEAVE, TIMING, EXPECT_RETRY = 1, 2, 4
NS_TLIST_SMALL = 1


class Writer:
    def __init__(self, out):
        self.out, self.count, self.names = out, 0, set()
        os.makedirs(out, exist_ok=True)

    def add(self, name, prog, grid=None, t=None, kind=COMPILE, nthreads=0, geom=(0, 0), keep_mixed_short=False,
            no_short_fmul=False, tlist_ns=0, env=None, baseline='', flags=0):
        assert name not in self.names and ' ' not in name, name
        self.names.add(name)

        def s(text):
            b = text.encode()
            return struct.pack('<i', len(b)) + b
        env = env or {}
        blob = [b'WFKIMG01', struct.pack('<8i', kind, nthreads, geom[0], geom[1], int(keep_mixed_short), int(no_short_fmul),
                                         tlist_ns, flags), s(baseline), struct.pack('<i', len(env))]
        for k in sorted(env):
            blob += [s(k), s(env[k])]
        g = grid if grid is not None else _flatten.wfk_grid()
        blob.append(struct.pack('<iddqidq', int(grid is not None), g.t0, g.step, int(g.n), int(g.has_last), g.last, int(g.i0)))
        t = np.zeros(0) if t is None else np.ascontiguousarray(t, dtype=np.float64)
        blob += [struct.pack('<q', len(t)), t.tobytes()]
        st = prog.struct
        blob.append(struct.pack('<5iq', st.n_channels, st.n_members, st.n_pieces, st.n_terms, st.n_factors, st.n_pool))
        for a in ARRAYS:
            arr = prog.arrays[a]
            assert arr.dtype == DTYPES.get(a, np.float64) and arr.flags.c_contiguous, (a, arr.dtype)
            blob += [struct.pack('<q', arr.nbytes), arr.tobytes()]
        with open(os.path.join(self.out, '%04d_%s.case' % (self.count, name)), 'wb') as f:
            f.write(b''.join(blob))
        self.count += 1

    def both(self, name, chans, gd, rng, **kw):
        """The plan on its grid, and on a jittered, sorted copy of (the first 4000 points of) the grid as a time list."""
        prog = _flatten.flatten(chans)
        grid = gd if isinstance(gd, _flatten.wfk_grid) else _flatten.grid_from_desc(gd)
        self.add(name + '.grid', prog, grid=grid, **kw)
        n = min(int(grid.n), 4000)
        t = np.sort(np.linspace(grid.t0, grid.t0 + grid.step * max(n - 1, 0), n) + rng.normal(size=n) * grid.step * 0.3) if n else np.zeros(0)
        self.add(name + '.tlist', prog, t=t, **kw)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('out')
    ap.add_argument('--random', type=int, default=300)
    a = ap.parse_args()
    w = Writer(a.out)
    rng = np.random.default_rng(2026)

    # ---- the sampler plans, each with its environment ----
    for key in sorted(tkn.PLANS):
        chans, gd, t, env = tkn.PLANS[key]()
        w.add('sampler.' + key, _flatten.flatten(chans), grid=None if gd is None else tkn._grid(gd), t=t, env=env)

    # ---- the case sets, as grids and as time lists ----
    for name, (build, gd) in cases.CASES.items():
        w.both('cases.' + name, [build(wf)], gd, rng)
    for name, (build, rate, n) in cases.AWG_CASES.items():
        for nn in (n, n // 3 + 1, 17):
            w.both('awg.%s.%d' % (name, nn), [build(wf, rate)], cases._awg_grid(nn, rate), rng)
    for seed in range(40):
        chans, gd = cases.far_from_origin_case(wf, seed)
        w.both('far.%d' % seed, chans, gd, rng)

    # (the fine-grid list, the edge grids and the malformed edits below are tools/sanitize/run_sanitized.py's, restated: that
    #  driver loads a sanitized library into Python and is left as it is -- a case added there belongs here too)
    def tones(nt):
        out = None
        for _ in range(nt):
            t = rng.uniform(0.05, 0.3) * wf.cos(2 * np.pi * rng.uniform(-3e8, 3e8), rng.uniform(0, 6))
            out = t if out is None else out + t
        return out
    W = 40e-9
    fine = [wf.square(W, edge=5e-9) >> 60e-9,
            (wf.square(W, edge=5e-9) >> 60e-9) * tones(10),
            (wf.square(W, edge=5e-9) >> 60e-9) * tones(14) * (0.3 - 0.4j),
            (wf.square(6e-9, edge=5e-9) >> 60e-9) * tones(3),
            wf.mixing(wf.square(W, edge=6e-9) >> 60e-9, freq=1.3e8, phase=0.2, DRAGScaling=2e-10)[0],
            (wf.square(W, edge=5e-9) * wf.gaussian(2 * W) * tones(2)) >> 60e-9,
            wf.coshPulse(W, eps=3.0, plateau=10e-9) >> 60e-9,
            (wf.square(W) >> 60e-9) * (wf.exp(-3e7) >> 20e-9) * tones(2),
            (wf.gaussian(W) >> 60e-9) * (wf.exp(4e7) >> 60e-9) * (wf.sinh(1e7) >> 50e-9),
            (wf.square(W) >> 60e-9) * wf.exp(1e11),
            (wf.gaussian(W) >> 60e-9) * tones(16)]
    fine_grids = (('linspace', 0.0, 120e-9, 400001, False), ('linspace', 1e-3, 1e-3 + 120e-9, 300000, True),
                  ('linspace', 0.0, 120e-9, 2001, False))
    for gi, gd in enumerate(fine_grids):
        for k in range(0, len(fine), 3):
            w.both('fine.%d.%d' % (gi, k), [c >> gd[1] for c in fine[k:k + 3]], gd, rng)
    for i in range(a.random):
        ch, gd = cases.random_channel(wf, rng)
        w.both('random.%d' % i, [ch], gd, rng)
    nine = [cases.random_channel(wf, rng)[0] for _ in range(9)]
    for gi, gd in enumerate((('linspace', 0.0, 1e-6, 0, True), ('linspace', 0.0, 1e-6, 1, True), ('linspace', 0.0, 1e-6, 2, False),
                             ('linspace', -3e-6, 5e-6, 70001, True), ('arange', -1e-6, 2e-6, 1e-9), ('arange', 0.0, 0.0, 1e-9))):
        w.both('edge_grid.%d' % gi, nine, gd, rng)

    # ---- request switches: a baseline and a witness whose image the switch changes ----
    awg = wl.awg_channel(wf, 0, 20000, 2e9)
    AWG = _flatten.grid_from_desc(wl.awg_grid(20000, 2e9))
    mixed_short = _flatten.flatten([awg + ((wf.sinc(2e8) * wf.square(600e-9)) >> 5e-6)])
    short_chirp = _flatten.flatten([awg + (wf.chirp(1e8, 2e8, 30e-9) >> 5e-6)])
    short_table = _flatten.flatten([awg + (wf.samplingPoints(-2e-8, 2e-8, np.hanning(50)) * wf.cos(2e9) >> 5e-6)])
    w.add('request.mixed_short.base', mixed_short, grid=AWG)
    w.add('request.mixed_short.keep_mixed_short', mixed_short, grid=AWG, keep_mixed_short=True, baseline='request.mixed_short.base')
    w.add('request.mixed_short.chain', mixed_short, grid=AWG, keep_mixed_short=True, no_short_fmul=True, tlist_ns=NS_TLIST_SMALL,
          flags=INTERLEAVE)                                           # (the compile that runs between the cases of the second pass)
    w.add('request.short_chirp.base', short_chirp, grid=AWG)
    w.add('request.short_chirp.no_short_fmul', short_chirp, grid=AWG, no_short_fmul=True, baseline='request.short_chirp.base')
    w.add('request.short_chirp.chain', short_chirp, grid=AWG, no_short_fmul=True, keep_mixed_short=True, baseline='request.short_chirp.base')
    w.add('request.short_table.base', short_table, grid=AWG)
    w.add('request.short_table.no_short_fmul', short_table, grid=AWG, no_short_fmul=True, baseline='request.short_table.base')
    big_t = tkn._jitter(tkn.BIG, 6 * wl.SPAN)                        # (tlist_ns shows only from WFK_TLIST_SMALL_N points on)
    six = _flatten.flatten([wl.sum_channel(wf, 6, 1000)])
    w.add('request.tlist_big.base', six, t=big_t)
    w.add('request.tlist_big.tlist_ns', six, t=big_t, tlist_ns=NS_TLIST_SMALL, baseline='request.tlist_big.base')
    # the grid plan that gives up and is compiled again pointwise, with the chain's request riding along
    gave_up = tkn.PLANS['grid_as_tlist']()
    w.add('request.grid_as_tlist.chain', _flatten.flatten(gave_up[0]), grid=tkn._grid(gave_up[1]), keep_mixed_short=True, no_short_fmul=True)

    # ---- ladder branches the sampler plans do not take ----
    far_chans, far_gd = tkn._far()
    tc = 16e-3
    w.add('ladder.lean_fam2_far', _flatten.flatten([far_chans[0] + (wf.chirp(1e8, 2e8, 300e-9) >> (tc - 0.5e-6))]), grid=tkn._grid(far_gd))
    w.add('ladder.lean_fam2_far_general', _flatten.flatten([far_chans[0] + (wf.chirp(1e8, 2e8, 300e-9) >> (tc - 0.5e-6))
                                                            + ((0.1 * wf.sinc(2e8) * wf.square(300e-9)) >> (tc + 0.5e-6))]), grid=tkn._grid(far_gd))
    for i, t_far in enumerate((2e-4, 1e-3, 4e-3)):     # (nearer the origin, where the chirp still fuses)
        ch, gd = tkn._far(t_center=t_far, f=900e6)
        w.add('ladder.lean_fam2_far.%d' % i, _flatten.flatten([ch[0] + (wf.chirp(1e8, 2e8, 300e-9) >> (t_far - 0.5e-6))]), grid=tkn._grid(gd))
    cs_chans, cs_gd = tkn._corr_short()
    w.add('ladder.short_corr_chirp', _flatten.flatten([cs_chans[0] + (wf.chirp(1e8, 2e8, 30e-9) >> (1e-3 + 3.5e-6))]), grid=tkn._grid(cs_gd))
    w.add('ladder.short_corr_table', _flatten.flatten([cs_chans[0] + (wf.samplingPoints(-2e-8, 2e-8, np.hanning(50)) >> (1e-3 + 3.5e-6))]),
          grid=tkn._grid(cs_gd))
    w.add('ladder.far_general', _flatten.flatten([far_chans[0] + ((0.1 * wf.sinc(2e8) * wf.square(300e-9)) >> (tc + 0.5e-6))]), grid=tkn._grid(far_gd))
    far_sinc = _flatten.flatten([far_chans[0] + ((0.1 * wf.sinc(2e8) * wf.square(300e-9)) >> (tc + 0.5e-6))])
    w.add('ladder.far_general_unmixed', far_sinc, grid=tkn._grid(far_gd), env={'WFK_DISABLE_MIXED': '1'})     # corrected, neither lean nor mixed: libm instead
    # a short plan far from t = 0: a few fast carriers among plain Gaussians, next to a chirp / a table (no short family holds both)
    t0 = 1e-3
    few = wf.zero()
    for k in range(100):
        g = wf.gaussian(20e-9)
        if k % 20 == 7:
            g = wf.mixing(g, freq=2.1e8 + 1e6 * k, phase=0.3, DRAGScaling=1e-10)[0]
        few = few + ((0.5 * g) >> (t0 + (k + 0.5) * 30e-9))
    w.add('ladder.short_needs_corr_chirp', _flatten.flatten([few + (wf.chirp(1e8, 2e8, 30e-9) >> (t0 + 3.5e-6))]), grid=tkn._grid(cs_gd))
    w.add('ladder.short_needs_corr_table', _flatten.flatten([few + (wf.samplingPoints(-2e-8, 2e-8, np.hanning(50)) >> (t0 + 3.5e-6))]), grid=tkn._grid(cs_gd))
    # a far carrier and a chirp in ONE piece (the last attempt of the ladder, no chirp and no correction, is reached by no plan we found)
    t1, g1 = 1e-3, tkn._grid(tkn._far(t_center=1e-3)[1])
    one_piece = (wf.square(300e-9) >> t1) * wf.cos(2 * np.pi * 900e6) + (wf.chirp(1e8, 2e8, 300e-9) >> (t1 - 150e-9))
    w.add('ladder.far_chirp_one_piece', _flatten.flatten([one_piece]), grid=g1)
    w.add('ladder.far_chirp_one_piece_sinc', _flatten.flatten([one_piece + ((0.1 * wf.sinc(2e8) * wf.square(300e-9)) >> t1)]), grid=g1)

    # ---- wfk_compile_geom at the two chain geometries ----
    smoke = _flatten.flatten([wl.sum_channel(wf, 6, 1000 + c) for c in range(4)])
    flat = _flatten.flatten(tkn._flat_tops())
    for ns in (28, 26):
        w.add('geom.lean.%d' % ns, smoke, grid=_flatten.grid_from_desc(('linspace', 0.0, 6 * wl.SPAN, 200000, False)), kind=GEOM, geom=(256, ns))
        w.add('geom.awg.%d' % ns, _flatten.flatten([awg]), grid=AWG, kind=GEOM, geom=(256, ns))
        w.add('geom.flat_tops.%d' % ns, flat, grid=_flatten.grid_from_desc(('linspace', 0.0, 1.2e-6, 60000, False)), kind=GEOM, geom=(256, ns))
    w.add('geom.scan.32', smoke, grid=_flatten.grid_from_desc(('linspace', 0.0, 6 * wl.SPAN, 200000, False)), kind=GEOM, geom=(1, 32))

    # ---- wfk_compile_blocks ----
    GA = _flatten.grid_from_desc(wl.awg_grid(6000, 2e9))
    GL = _flatten.grid_from_desc(('linspace', 0.0, 40 * wl.SPAN, 300000, False))
    batches = {}
    for nch in (16, 33):
        batches['awg%d' % nch] = (_flatten.flatten([wl.awg_channel(wf, c, 6000, 2e9, c % 3 == 0) for c in range(nch)]), GA)
        batches['lean%d' % nch] = (_flatten.flatten([wl.sum_channel(wf, 40, 50 + c) for c in range(nch)]), GL)
    batches['awg_tables16'] = (_flatten.flatten([wl.awg_interp_channel(wf, c, 6000, 2e9) if c % 2 else wl.awg_shape_channel(wf, 'flat_top', c, 6000, 2e9)
                                                 for c in range(16)]), GA)
    lean15 = [wl.sum_channel(wf, 40, 50 + c) for c in range(15)]
    batches['erf_edge16'] = (_flatten.flatten(lean15 + [(wf.square(400e-9, edge=50e-9) >> 1e-6) * wf.cos(2 * np.pi * 50e6) + wl.sum_channel(wf, 40, 3)]), GL)
    # batches wfk_compile_blocks hands back (WFK_RETRY_STD, the caller compiles in one piece; the image program FAILS if one of
    # them stops doing so): a lean block with a pool table, a block that comes out mixed, a lean block beside short ones
    retries = {
        'retry_pool16': (_flatten.flatten(lean15 + [wl.sum_channel(wf, 40, 3) + ((tkn._hann(200) * wf.cos(2e9)) >> 0.6e-6)]), GL),
        'retry_mixed16': (_flatten.flatten(lean15 + [wl.sum_channel(wf, 40, 3) + ((0.1 * wf.sinc(2e8) * wf.square(300e-9)) >> 0.6e-6)]), GL),
        'retry_tiers16': (_flatten.flatten([wl.awg_channel(wf, c, 6000, 2e9) for c in range(8)] +
                                           [(wf.gaussian(2e-6) >> 1.5e-6) * wf.cos(2 * np.pi * (40e6 + 1e6 * c)) for c in range(8)]), GA),
    }
    bad = _flatten.flatten([wl.awg_channel(wf, c, 6000, 2e9) for c in range(16)])
    bad.arrays['fc_type'] = bad.arrays['fc_type'].copy()
    bad.arrays['fc_type'][-1] = 99                                    # an id without a device form, in the LAST block
    batches['invalid16'] = (bad, GA)
    for name, (prog, grid) in batches.items():
        for nt in (2, 3, 4):
            w.add('blocks.%s.t%d' % (name, nt), prog, grid=grid, kind=BLOCKS, nthreads=nt)
        w.add('blocks.%s.whole' % name, prog, grid=grid)
    for name, (prog, grid) in retries.items():
        for nt in (2, 3, 4):
            w.add('blocks.%s.t%d' % (name, nt), prog, grid=grid, kind=BLOCKS, nthreads=nt, flags=EXPECT_RETRY)
        w.add('blocks.%s.whole' % name, prog, grid=grid)                                  # (what the caller then compiles ...
        w.add('blocks.%s.whole.chain' % name, prog, grid=grid, keep_mixed_short=True, no_short_fmul=True)   # ... with the request it was given)
    w.add('blocks.awg16.t4.chain', batches['awg16'][0], grid=GA, kind=BLOCKS, nthreads=4, keep_mixed_short=True, no_short_fmul=True)
    w.add('blocks.awg16.t4.upc', batches['awg16'][0], grid=GA, kind=BLOCKS, nthreads=4, env={'WFK_SH_UPC': '2'}, baseline='blocks.awg16.t4')
    w.add('blocks.lean16.t4.tpc', batches['lean16'][0], grid=GL, kind=BLOCKS, nthreads=4, env={'WFK_TPC': '3'}, baseline='blocks.lean16.t4')

    # ---- environment switches: every one on a plan it affects (a witness against the sampler plan without it) ----
    def env_case(var, value, key, grid=None, chans=None):
        """`key`: a sampler plan (its case above is the baseline), or with `chans` a plan of our own, whose baseline is added once."""
        if chans is None:
            chans, gd, t, env = tkn.PLANS[key]()
            assert not env
            grid, base = None if gd is None else tkn._grid(gd), 'sampler.' + key
        else:
            t, base = None, 'env.base.' + key
            if base not in w.names:
                w.add(base, _flatten.flatten(chans), grid=grid)
        w.add('env.%s=%s.%s' % (var, value, key), _flatten.flatten(chans), grid=grid, t=t, env={var: value}, baseline=base)
    FINE = _flatten.grid_from_desc(tkn.FINE)
    env_case('WFK_NO_SINC_TAB', '1', 'general_direct')
    env_case('WFK_NO_MOLL_REC', '1', 'moll_fine', FINE, [(wf.mollifier(40e-9) * wf.sinc(2e8)) >> 60e-9])   # (generic terms: factor by factor)
    interp_fine = [(tkn._hann(200) * wf.sinc(2e8)) >> 60e-9]
    env_case('WFK_NO_INTERP_GRID', '1', 'interp_fine', FINE, interp_fine)
    env_case('WFK_NO_INTERP_LIN', '1', 'interp_fine', FINE, interp_fine)
    w.add('env.WFK_NO_SHORT_CMUL=1.short_table', short_table, grid=AWG, env={'WFK_NO_SHORT_CMUL': '1'}, baseline='request.short_table.base')
    env_case('WFK_NO_SHORT_CHIRP', '1', 'short_fam1')
    hann50 = wf.samplingPoints(-2e-8, 2e-8, np.hanning(50))
    env_case('WFK_NO_SHORT_MULTI', '1', 'short_two_tables', AWG, [((hann50 * wf.cos(2e9)) >> 5e-6) + ((0.5 * wf.samplingPoints(-2e-8, 2e-8, np.hanning(41)) * wf.cos(1.5e9)) >> 5.01e-6)])
    env_case('WFK_NO_LEAN_MULTI', '1', 'lean_fam4')
    env_case('WFK_NO_SHORT_ENVMUL', '1', 'short_envmul', AWG, [tkn._pulse_train(lambda k, r: wf.gaussian(40e-9) * tones(5), 50, 60e-9)])
    env_case('WFK_NO_BANK', '1', 'lean_fam1')
    env_case('WFK_NO_SHORT_XCHIRP', '1', 'short_fam4')
    env_case('WFK_NO_SHORT_ERFTAB', '1', 'short_fam2')
    env_case('WFK_NO_SHORT_CORR', '1', 'short_fam6')
    w.add('env.WFK_KEEP_MIXED_SHORT.mixed_short', mixed_short, grid=AWG, env={'WFK_KEEP_MIXED_SHORT': '1'}, baseline='request.mixed_short.base')
    env_case('WFK_TLSMALL_LIMIT', '1.0', 'tlist_fused_small')
    env_case('WFK_DISABLE_FAST', '1', 'lean_fam0')
    env_case('WFK_DISABLE_CORR', '1', 'lean_corr0')
    env_case('WFK_DISABLE_CHIRP', '1', 'lean_fam2')
    env_case('WFK_DISABLE_LEAN', '1', 'lean_fam0')
    env_case('WFK_DISABLE_FUSE', '1', 'lean_fam0')
    env_case('WFK_DISABLE_TLFUSE', '1', 'tlist_fused_small')
    env_case('WFK_DISABLE_EXPFUSE', '1', 'exp_fine', _flatten.grid_from_desc(fine_grids[0]), fine[7:9])
    env_case('WFK_DISABLE_ERFMUL', '1', 'lean_corr1')
    env_case('WFK_DISABLE_FMUL', '1', 'lean_fam3')
    env_case('WFK_DISABLE_MIXED', '1', 'lean_general')
    env_case('WFK_SHORT', '0', 'short_fam0')
    env_case('WFK_SHORT', '1', 'lean_fam0')
    env_case('WFK_SHORT_MAXLEN', '10', 'short_fam0')
    env_case('WFK_TPC', '3', 'lean_fam0')
    w.add('env.WFK_TPC=99.lean_fam0', _flatten.flatten(tkn.PLANS['lean_fam0']()[0]), grid=FINE, env={'WFK_TPC': '99'})   # (out of range: ignored)
    # (the float launch has a chunk table of its own only from ~150 k lean tiles on: 4 rows of 5e7 samples; the compile is O(pieces))
    env_case('WFK_TPC_F32', '6', 'lean_long', _flatten.grid_from_desc(('linspace', 0.0, 6 * wl.SPAN, 50_000_000, False)),
             [wl.sum_channel(wf, 6, 1000 + c) for c in range(4)])
    env_case('WFK_SH_UPC', '2', 'short_fam0')

    # ---- malformed programs: refused, with the same code and text ----
    def broken(k, edit):
        p = _flatten.flatten([wf.gaussian(0.5) * wf.cos(3.0) >> 0.5, wf.square(0.3) * 2 + wf.sinc(4.0)])
        edit(p)
        w.add('malformed.%d' % k, p, grid=_flatten.grid_linspace(0.0, 1.0, 100))

    def e1(p): p.arrays['pc_term_off'][1] = 99
    def e2(p): p.arrays['pc_bound'][-1] = 1.0
    def e3(p): p.arrays['pc_bound'][0], p.arrays['pc_bound'][1] = 5.0, -5.0
    def e4(p): p.arrays['fc_arg_off'][-1] += 1
    def e5(p): p.arrays['fc_type'][0] = 99
    def e6(p): p.arrays['ch_clip_lo'][0] = float('nan')
    def e7(p): p.arrays['tm_factor_off'][-1] = 10**6
    def e8(p): p.arrays['ch_member_off'][1] = 7
    def e9(p): p.arrays['mb_piece_off'][1] = 0
    def e10(p): p.arrays['fc_arg_off'][1] = -3
    def e11(p): p.struct.n_terms = -1
    def e12(p): p.struct.n_pool = 10**7
    for k, e in enumerate((e1, e2, e3, e4, e5, e6, e7, e8, e9, e10, e11, e12), 1):
        broken(k, e)
    w.add('malformed.grid_step', _flatten.flatten([wf.gaussian(0.5)]), grid=_flatten.wfk_grid(0.0, -1.0, 10, 0, 0.0))
    w.add('malformed.grid_i0', _flatten.flatten([wf.gaussian(0.5)]), grid=_flatten.wfk_grid(0.0, 1.0, 10, 0, 0.0, -1))

    # ---- branches of the piece loop that none of the lists above takes ----
    FINE_G = _flatten.grid_from_desc(tkn.FINE)
    sq = wf.square(W) >> 60e-9
    # direct-factor records: a Gaussian derivative next to a factor that does not fuse (the term stays generic) ...
    for d in (1, 2):
        w.both('reach.direct_dgauss.%d' % d, [(wf.gaussian(W, d=d) * wf.sinc(2e8)) >> 60e-9], tkn.FINE, rng)
    # ... and a caller-evaluated factor: one table, its member piece cut into three device pieces by a second member
    unit = _flatten.grid_linspace(-3.0, 3.0, 4001)
    tanh = wf.function(np.tanh, start=-2, stop=2) * wf.cos(3.0)
    w.add('reach.direct_sampled', _flatten.flatten([tanh], axis=unit), grid=unit)
    stack = wf.WaveVStack([tanh, 0.5 * (wf.square(1.0) >> 0.25) * wf.sinc(2.0)])
    w.add('reach.direct_sampled_shared', _flatten.flatten([stack], axis=unit), grid=unit)
    # more generic terms than one LDS block holds: the piece is cut into several blocks
    many = wf.zero()
    for k in range(70):
        many = many + 0.01 * wf.sinc(1e8 + 1e6 * k) * wf.cos(2 * np.pi * (2e7 + 3e6 * k))
    w.both('reach.blocks_overflow', [sq * many], tkn.FINE, rng)
    # a chirp multiplied by a carrier, in both orders, and by two
    CH = ('linspace', 0.0, 500e-9, 50000, False)
    chirp = wf.chirp(1e8, 2e8, 300e-9) >> 100e-9
    w.both('reach.chirp_carrier', [chirp * wf.cos(2 * np.pi * 5e7, 0.3)], CH, rng)
    w.both('reach.carrier_chirp', [wf.cos(2 * np.pi * 5e7, 0.3) * chirp + (wf.gaussian(20e-9) >> 50e-9)], CH, rng)
    w.both('reach.chirp_two_carriers', [chirp * wf.cos(2 * np.pi * 5e7) * wf.cos(2 * np.pi * 3e7, 1.0)], CH, rng)
    # an exponential of its own under a power of t (its rate weighed with the term's amplitude); rates that cancel to a constant
    ramp = wf.poly([0.5, 1e7]) >> 60e-9
    w.both('reach.exp_linear', [sq * (wf.exp(-3e7) >> 20e-9) * ramp, 40.0 * sq * (wf.exp(9e7) >> 20e-9) * ramp * ramp], tkn.FINE, rng)
    w.both('reach.exp_cancels', [sq * (wf.exp(-3e7) >> 20e-9) * (wf.exp(3e7) >> 50e-9) * tones(2),
                                 sq * (wf.cosh(2e7) >> 50e-9) * (wf.exp(2e7) >> 55e-9)], tkn.FINE, rng)
    # a product of three DRAG pulses: more carriers than a term may expand into (it stays generic)
    d3 = wf.drag(2e8, W, delta=1e6, block_freq=3e8) * wf.drag(1.5e8, W, phase=0.4) * wf.drag(1e8, W, delta=-2e6)
    w.both('reach.carriers_overflow', [d3 >> 40e-9], tkn.FINE, rng)
    # 36 tones under two Gaussians in turn: more per-lane state than a lean block has units
    wide_state = wf.zero()
    for k in range(36):
        wide_state = wide_state + 0.03 * wf.gaussian(W + 2e-9 * (k % 2)) * wf.cos(2 * np.pi * (2e7 + 5e6 * k))
    w.both('reach.state_units', [wide_state >> 60e-9], tkn.FINE, rng)
    # refused: one generic term of more factors than the LDS parameter buffer takes
    wide = sq
    for k in range(50):
        wide = wide * (wf.sinc(1e8 + 1e6 * k) >> (60e-9 + 1e-10 * k))
    w.add('reach.term_too_wide', _flatten.flatten([wide]), grid=FINE_G)

    # ---- the timing workloads (plan_image --time) ----
    G1 = _flatten.grid_from_desc(wl.awg_grid(100000, 2e9))
    w.add('time.awg_channel', _flatten.flatten([wl.awg_channel(wf, 0, 100000, 2e9)]), grid=G1, flags=TIMING)
    batch16 = _flatten.flatten([wl.awg_channel(wf, c, 100000, 2e9, c % 3 == 0) for c in range(16)])
    w.add('time.awg_batch16', batch16, grid=G1, flags=TIMING)
    batch33 = _flatten.flatten([wl.awg_channel(wf, c, 100000, 2e9, c % 3 == 0) for c in range(33)])
    w.add('time.awg_blocks33.t4', batch33, grid=G1, kind=BLOCKS, nthreads=4, flags=TIMING)
    print('%d cases in %s' % (w.count, a.out))


if __name__ == '__main__':
    main()
