/*
 * wfk.h -- C-ABI of the MI355X waveform-sampling engine (libwfk_hip.so).
 *
 * This is the drop-in boundary for ONE hot path of feihoo87/waveforms:
 *   piecewise sum-of-products expression tree  ->  dense sample array
 * i.e. what the reference does inside
 *   calc_parts()            waveforms/_waveform.pyx:155-169   (+ _calc :134-152, _apply :130-131)
 *   Waveform._fill_parts()  waveforms/waveform.py:524-527
 *   Waveform.__call__()     waveforms/waveform.py:529-563
 *   WaveVStack.__call__()   waveforms/waveform.py:679-693
 *   Waveform.sample()       waveforms/waveform.py:173-207    (np.arange grid)
 *   predistort(ker=...)     waveforms/distortion.py:323-337  (FIR branch)
 *
 * Plain C: pointers and sizes only, no torch / HIP types.  Every function
 * returns 0 on success or a negative WFK_E* code; wfk_last_error() returns a
 * thread-local message.  The caller owns every host buffer and every opaque
 * handle (explicit *_destroy); the library owns device tables inside a plan.
 * wfk_plan_launch() and wfk_fir_apply() allocate nothing and do not synchronise.
 *
 * Graph capture.  Every entry whose comment says that it "allocates nothing and does not synchronise" -- in these
 * words -- enqueues kernels, memsets and device-to-device copies on `hip_stream` and does nothing else to the device,
 * so it may be called while that stream is being captured (hipStreamBeginCapture, torch.cuda.graph) and the graph
 * replayed once per shot: wfk_plan_launch, wfk_fir_apply, wfk_chain_launch, wfk_iir_apply, wfk_iir_rows_apply,
 * wfk_chain_iir_launch, wfk_chain_iir_rows_launch, wfk_spectral_apply, wfk_spectral_rows_apply, wfk_shift_rows_apply,
 * wfk_dac_rows_apply, wfk_marker_rows_apply, wfk_marker_rows_apply_codes, wfk_mix_rows_apply, wfk_extract_rows_apply,
 * wfk_demod_apply and wfk_boxprobe_apply.  Creation, destruction, *_run_host, wfk_iir_status and wfk_chain_iir_status
 * allocate or synchronise and must stay outside a capture.
 * A capture freezes what the call was given and what it decided: every pointer and stride (feed a replay by copying
 * into the captured buffers), the scalar `initial` of the IIR entries, `bit` of wfk_marker_rows_apply_codes, `flags`
 * and `out_kind`, and the environment switches an entry reads when it launches (WFK_IIR_SPIN, WFK_IIR_OP_DEPTH).
 * Device arrays -- zi, the per-row initial_dev, an accumulate base -- are read anew by every replay; zf, counts and
 * every other output are written anew, never accumulated across replays.  No launch depends on how many went before.
 * A look-back time-out of the single-pass IIR during a REPLAY is reported by wfk_iir_status / wfk_chain_iir_status
 * alone (the replay calls no entry that could return WFK_ETIMEOUT); the graph keeps launching the single-pass form, so
 * capture again after it.  "One plan per concurrent stream" also means: a plan that owns scratch is not in two graphs
 * that replay at the same time, nor in a graph replaying while the plan is applied eagerly on another stream.
 */
#ifndef WFK_H
#define WFK_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define WFK_ABI_VERSION 2   /* 2: wfk_grid.i0 (time slices of a grid) */

/* error codes */
#define WFK_OK 0
#define WFK_EINVAL (-1)   /* malformed program / argument                      */
#define WFK_EUNSUP (-2)   /* primitive id without a device implementation      */
#define WFK_EHIP   (-3)   /* HIP runtime / rocFFT failure                      */
#define WFK_ENOMEM (-4)
#define WFK_ETIMEOUT (-5)  /* a chained device-side wait ran out of polls (IIR single pass)   */

/* Primitive ids == the reference registry (waveforms/_waveform.pyx:374-388).
 * args (in `pool`, at fc_arg_off) per id, evaluated at u = t - shift:
 *   1 LINEAR            ()                      u
 *   2 GAUSSIAN          (std_sq2)               exp(-(u/std_sq2)^2)                 pyx:294-295
 *   3 ERF               (std_sq2)               erf(u/std_sq2)                      pyx:303-304
 *   4 COS               (w)                     cos(w*u)                            pyx:307-308
 *   5 SINC              (bw)                    np.sinc(bw*u)                       pyx:311-312
 *   6 EXP               (alpha)                 exp(alpha*u)                        pyx:315-316
 *   7 INTERP            (start, stop, p0..pm-1) np.interp(u, linspace(start,stop,m), p)   pyx:319-320
 *   8 LINEARCHIRP       (f0, f1, T, phi0)       pyx:323-324
 *   9 EXPONENTIALCHIRP  (f0, alpha, phi0)       pyx:327-328
 *  10 HYPERBOLICCHIRP   (f0, k, phi0)           pyx:331-332
 *  11 COSH (w)  12 SINH (w)                     pyx:335-340
 *  13 DRAG              (t0, freq, width, delta, block_freq|NaN=None, phase)        pyx:343-356
 *  14 MOLLIFIER         (r, d)                  pyx:359-371
 *  15 D_GAUSSIAN        (std_sq2, n)            pyx:298-300
 *  16 DRAG_SIN / 17 DRAG_SINX  multi-notch DRAG (waveforms/multy_drag.py:158-213), args in
 *     COMPILED form (the per-pulse matrices folded into coefficient tables on the host,
 *     waveforms_amd/multy_drag.py:device_args):
 *       (t0, freq, width, delta, phase, plateau, tab_half_width, m, dq,
 *        Px[0..m], Py[0..m], Cx, Cy [, QLx, QLy, QRx, QRy (dq+1 each, highest power first)])
 * 1000 SAMPLED (i0, v[0..m-1]): the factor's value at sample index j is v[j - i0] (j - i0
 *     clamped into [0, m)); `shift` is ignored.  This is how a primitive that only the CALLER
 *     can evaluate reaches the device: the caller evaluates it once per distinct factor on the
 *     plan's own time axis, over the samples of the piece (i0 = first sample of the piece), exactly
 *     where the reference calls function_lib[id](x[start:stop] - shift, *args)
 *     (_apply, waveforms/_waveform.pyx:130-131) -- Python callables registered with function() /
 *     registerBaseFunc (waveform.py:1470-1478, _waveform.pyx:264-271) and function_lib= overrides
 *     (waveform.py:178,535,679).
 * Any other id -> WFK_EUNSUP.                                                     */
enum {
  WFK_LINEAR = 1, WFK_GAUSSIAN = 2, WFK_ERF = 3, WFK_COS = 4, WFK_SINC = 5,
  WFK_EXP = 6, WFK_INTERP = 7, WFK_LINEARCHIRP = 8, WFK_EXPONENTIALCHIRP = 9,
  WFK_HYPERBOLICCHIRP = 10, WFK_COSH = 11, WFK_SINH = 12, WFK_DRAG = 13,
  WFK_MOLLIFIER = 14, WFK_D_GAUSSIAN = 15, WFK_DRAG_SIN = 16, WFK_DRAG_SINX = 17,
  WFK_SAMPLED = 1000
};

/*
 * Flattened expression forest (struct-of-arrays, depth-first in the order of
 * the reference's own flattener Waveform._tolist, waveforms/waveform.py:259-276):
 *
 *   channel  = one output row.  A `Waveform` is a channel with ONE member and
 *              its min/max as clip; a `WaveVStack` is a channel with one member
 *              per wlist entry, `offset`, `shift`, and clip = -inf/+inf.
 *   member   = (bounds, seq): pieces in ascending bound order, last bound +inf.
 *              piece i is live for bound[i-1] <= t - tshift < bound[i]
 *              (np.searchsorted side='left', _waveform.pyx:156).
 *   piece    = sum of terms;  term = amp * prod_j factor_j(t - tshift - shift_j)^power_j
 */
typedef struct wfk_program {
  int32_t n_channels, n_members, n_pieces, n_terms, n_factors;
  int64_t n_pool;
  const int32_t* ch_member_off;  /* [n_channels+1]                               */
  const double*  ch_offset;      /* [n_channels]  WaveVStack.offset (real part)  */
  const double*  ch_tshift;      /* [n_channels]  WaveVStack.shift               */
  const double*  ch_clip_lo;     /* [n_channels]  Waveform.min                   */
  const double*  ch_clip_hi;     /* [n_channels]  Waveform.max                   */
  const int32_t* mb_piece_off;   /* [n_members+1]                                */
  const double*  pc_bound;       /* [n_pieces]    upper bound in seconds         */
  const int32_t* pc_term_off;    /* [n_pieces+1]                                 */
  const double*  tm_amp_re;      /* [n_terms]                                    */
  const double*  tm_amp_im;      /* [n_terms]                                    */
  const int32_t* tm_factor_off;  /* [n_terms+1]                                  */
  const int32_t* fc_type;        /* [n_factors]   primitive id                   */
  const double*  fc_power;       /* [n_factors]                                  */
  const double*  fc_shift;       /* [n_factors]                                  */
  const int64_t* fc_arg_off;     /* [n_factors+1] into pool                      */
  const double*  pool;           /* [n_pool]                                     */
} wfk_program;

/* Uniform time grid, bit-identical to NumPy's:
 *   t[i] = fl(fl(i*step) + t0)           np.linspace / np.arange element formula
 *   t[n-1] = last  if has_last            np.linspace(endpoint=True) override
 * (replaces the `x` argument of Waveform.__call__ and the
 *  np.arange of Waveform.sample, waveforms/waveform.py:190,232).               */
typedef struct wfk_grid {
  double t0, step;
  int64_t n;
  int32_t has_last;
  double last;
  int64_t i0;      /* index of this grid's first sample in the caller's FULL grid: t[i] = fl(fl((i0 + i)*step) + t0).
                    * 0 for a whole grid; > 0 for a time slice of one (time-axis sharding, chunked sampling):
                    * the slice's samples and piece indices are then bit-identical to the same samples of the
                    * whole grid.  has_last refers to the slice's own last sample (set it only where the slice
                    * ends with the full grid's overridden last sample).                                     */
} wfk_grid;

enum { WFK_OUT_F64 = 0, WFK_OUT_F32 = 1, WFK_OUT_C128 = 2, WFK_OUT_C64 = 3 };

/* launch flags */
#define WFK_ACCUMULATE 1u   /* out += samples  (Waveform.__call__(accumulate=True)) */

typedef struct wfk_plan wfk_plan;
typedef struct wfk_fir_plan wfk_fir_plan;

typedef struct wfk_plan_info {
  int32_t n_channels;
  int64_t n;             /* samples per channel                                  */
  int32_t tile;          /* samples per workgroup tile                           */
  int64_t n_tiles;       /* workgroups per launch                                */
  int32_t n_pieces;      /* merged device pieces                                 */
  int64_t param_doubles; /* device parameter stream length                      */
  int32_t n_fast;        /* factor uses on a recurrence / table fast path        */
  int32_t n_direct;      /* factor uses evaluated with device libm               */
  int32_t n_fused;       /* terms absorbed into fused carrier-envelope ops       */
  int32_t n_generic;     /* terms evaluated factor by factor                     */
} wfk_plan_info;

int         wfk_abi_version(void);
const char* wfk_last_error(void);
int         wfk_device_count(int* count);
int         wfk_set_device(int ordinal);

/* -- sampler plans ------------------------------------------------------- */
/* grid mode: replaces calc_parts(bounds, seq, x=grid, ...) for every channel   */
int wfk_plan_create_grid(const wfk_program* prog, const wfk_grid* grid,
                         wfk_plan** out);
/* tlist mode: x is an explicit sorted float64 array on the host (it is
 * uploaded); replaces Waveform.__call__(x) for arbitrary x                     */
int wfk_plan_create_tlist(const wfk_program* prog, const double* t_host,
                          int64_t n, wfk_plan** out);
/* 1 and *grid filled if the sorted host array t_host[0..n) is BIT-IDENTICAL to a uniform NumPy
 * grid (np.linspace with or without endpoint, np.arange: every element is compared), else 0.
 * Lets Waveform.__call__(x) (waveform.py:529-563) compile grid mode for the usual x.     */
int wfk_grid_detect(const double* t_host, int64_t n, wfk_grid* grid);
/* The same for an x that is SEVERAL such grids back to back (np.concatenate of the chunks of a chunked job,
 * waveforms/waveform.py:232; a sequence sampled at two rates): number of runs found -- starts[k] = index of
 * run k's first sample, grids[k] its grid, every element verified -- or 0 (a run shorter than min_len,
 * more than max_runs runs, anything that is not exactly a grid).  The caller then samples run by run in grid
 * mode instead of handing the whole x over as a time list.                                                */
int wfk_grid_detect_runs(const double* t_host, int64_t n, int64_t min_len, int32_t max_runs,
                         int64_t* starts, wfk_grid* grids);
int wfk_plan_destroy(wfk_plan* plan);
int wfk_plan_get_info(const wfk_plan* plan, wfk_plan_info* info);
/* np.searchsorted(x - tshift, bounds) of one member (integer parity probe);
 * writes min(cap, #bounds) values, returns #bounds                            */
int wfk_plan_member_index(const wfk_plan* plan, int32_t member, int64_t* idx,
                          int32_t cap);
/* 1 if a live piece of `channel` has a complex amplitude (dtype detection of
 * calc_parts, _waveform.pyx:164-166)                                          */
int wfk_plan_channel_is_complex(const wfk_plan* plan, int32_t channel);
/* Name of the device kernel a launch of this plan with `out_kind` selects (the symbol
 * rocprofv3 --kernel-trace shows, template arguments included), for reports.           */
const char* wfk_plan_kernel_name(const wfk_plan* plan, int out_kind);
/* Bytes of device tables a launch of this plan reads (channels, pieces / units, parameter records,
 * slots, pool): at AWG sample rates (tens of samples per piece) they are a real share of the HBM
 * traffic next to the output stream, and bench.py reports them beside the algorithmic bytes.      */
int64_t wfk_plan_table_bytes(const wfk_plan* plan);
/* Evaluate every channel into out_dev[ch*ch_stride + i] (elements of out_kind).
 * Asynchronous on `hip_stream` (a hipStream_t, or NULL for the null stream).   */
int wfk_plan_launch(wfk_plan* plan, void* out_dev, int64_t ch_stride,
                    int out_kind, uint32_t flags, void* hip_stream);
/* launch into an internal device buffer, copy to out_host, synchronise         */
int wfk_plan_run_host(wfk_plan* plan, void* out_host, int64_t ch_stride,
                      int out_kind);

/* -- FIR stage: out[i] = sum_k ker[k] * sig[i + K/2 - k], zero padded ------- */
/* replaces predistort(sig, ker=ker), waveforms/distortion.py:329-337          */
/* Kernels of up to 6148 taps on up to 65535 rows run on the on-chip transform, whatever n.  Anything else runs on
 * the rocFFT pipeline, which holds one row in at most 65535 blocks of L - K + 1 samples (L the transform length,
 * the power of two >= 8 K, at least 1024): creation fails with WFK_EINVAL for a longer n, before anything is
 * allocated.                                                                                                    */
int wfk_fir_plan_create(const double* ker_host, int32_t K, int64_t n,
                        int32_t batch, int kind /* WFK_OUT_F64|F32 */,
                        wfk_fir_plan** out);
/* the same with one kernel PER ROW: kers_host[row * K + k] (every AWG line has its own predistortion kernel;
 * upstream the call is per signal anyway).  On-chip transform only: K <= 6148, batch <= 65535.          */
int wfk_fir_plan_create_rows(const double* kers_host, int32_t K, int64_t n,
                             int32_t batch, int kind /* WFK_OUT_F64|F32 */,
                             wfk_fir_plan** out);
/* Row r: n elements at in_dev + r * in_stride -> out_dev + r * out_stride (strides in elements, >= n).
 * OUT OF PLACE: workgroups read input that belongs to the blocks of others, and a long kernel reads `in` in
 * several passes.  WFK_EINVAL if [in, in + (batch-1)*in_stride + n) and [out, out + (batch-1)*out_stride + n)
 * share a byte.
 * Non-finite input: a NaN or Inf in sample p of row r reaches every output of row r that was computed in one
 * transform with it, and no other row.  That is at least out[r][p - K/2 .. p - K/2 + K) (the outputs whose sum has a
 * term on sample p; none of them is ever finite) and at most the output blocks of the windows that read sample p: on
 * the on-chip transform blocks of M = 4097 - Kseg samples (Kseg = K up to 1537 taps, else ceil(K / nseg) with nseg =
 * ceil(K / 1537) passes, pass j reading j * Kseg samples earlier), window b reading in[b M - lead, b M - lead + 4096),
 * lead = Kseg - 1 - K/2 + j Kseg, and taking the block of its pair partner b ^ 1 with it (two windows share one
 * complex transform): 6146 samples for K = 1024; on the rocFFT pipeline blocks of M = L - K + 1 samples, no partner.
 * Every output outside that span is bit for bit what it is without the bad sample.  (scipy's fftconvolve, one
 * transform per signal, loses the whole row.)                                                               */
int wfk_fir_apply(wfk_fir_plan* plan, const void* in_dev, int64_t in_stride,
                  void* out_dev, int64_t out_stride, void* hip_stream);
/* The form wfk_fir_apply runs: "fir_fused<T>" (" x N" behind it for a kernel cut into N accumulated passes,
 * " per-row spectra" for wfk_fir_plan_create_rows) or "fir_gather<T> + rocfft<L=..,rows=..> + fir_multiply<T> +
 * fir_scatter<T>" (transform length, rows per chunk); "" for n == 0.  The string belongs to the calling thread and
 * lasts until its next call.                                                                                */
const char* wfk_fir_kernel_name(const wfk_fir_plan* plan);
int wfk_fir_plan_destroy(wfk_fir_plan* plan);

/* -- sampler -> FIR chain (BASELINE configs[3]) --------------------------------- */
/* out = predistort(wav(t), ker=ker): Waveform.__call__ (waveforms/waveform.py:529-563) followed by
 * the FIR branch of predistort (waveforms/distortion.py:329-337), for every channel of `prog` on
 * `grid`.  When every piece of the program is fully fused (carrier-envelope ops only, no clip, real
 * amplitudes) and the kernel fits one on-chip transform (K <= 1537) the FIR workgroups EVALUATE
 * their input windows instead of loading them: the samples never touch HBM and the chain moves the
 * 8 (4) B/sample of the filtered output only.  At AWG sample rates (plans in the short geometry) the
 * windows are sampled the short tier's way (fir_short); pieces without a short form travel through a
 * sparsely written workspace.  Otherwise the plan owns a workspace and runs
 * sampler -> workspace -> FIR (wfk_chain_is_fused() == 0, wfk_chain_unfused_reason() says why).
 * Non-finite samples: a NaN or Inf that channel r's program evaluates to at sample p (a table envelope with a bad
 * knot) reaches row r as it does through wfk_fir_apply, and no other row -- fused, the windows hop 3072 samples (K <=
 * 1025) or 2560, window b reads samples [b hop - lead, b hop - lead + 4096), lead = K - 1 - K/2, and takes the block
 * of its pair partner with it; unfused, the geometry is that of wfk_fir_apply.
 * wfk_chain_launch() allocates nothing and does not synchronise.                              */
typedef struct wfk_chain_plan wfk_chain_plan;
int wfk_chain_plan_create(const wfk_program* prog, const wfk_grid* grid, const double* ker_host,
                          int32_t K, int kind /* WFK_OUT_F64|F32 */, wfk_chain_plan** out);
/* one kernel per channel: kers_host[channel * K + k] */
int wfk_chain_plan_create_rows(const wfk_program* prog, const wfk_grid* grid, const double* kers_host,
                               int32_t K, int kind /* WFK_OUT_F64|F32 */, wfk_chain_plan** out);
int wfk_chain_is_fused(const wfk_chain_plan* plan);
/* "fir_sampled<T,HOPB>" (stride-256 chains, fine grids), "fir_short<T,HOPB>" (contiguous lane runs, AWG
 * rates) or the two kernels of the unfused path; the string lives until the next call on this thread */
const char* wfk_chain_kernel_name(const wfk_chain_plan* plan);
/* bytes of device tables one launch reads besides the kernel spectrum (records, window entries) */
int64_t wfk_chain_table_bytes(const wfk_chain_plan* plan);
const char* wfk_chain_unfused_reason(const wfk_chain_plan* plan);
int wfk_chain_launch(wfk_chain_plan* plan, void* out_dev, int64_t out_stride, void* hip_stream);
int wfk_chain_plan_destroy(wfk_chain_plan* plan);

/* -- IIR stage ---------------------------------------- */
/* y = cascade of direct-form-II-transposed sections along each row, i.e.
 *   scipy.signal.sosfilt (n_sections sections of order 2)  -- Waveform.sample(filters=),
 *                                                             waveforms/waveform.py:193-203,244-251
 *   scipy.signal.lfilter (ONE section of order max(len(a),len(b))-1) -- predistort(filters=),
 *                                                             waveforms/distortion.py:298-321
 * orders[s] = order of section s; b and a hold the sections back to back, orders[s]+1
 * coefficients each (a[0] of a section need not be 1).  State layout == scipy's zi:
 * sections back to back, orders[s] values each (total wfk_iir_state_dim()).
 * apply: out = F(in - initial) + initial; zi_dev/zf_dev: optional [batch][state_dim]
 * device arrays (initial state in, final state out; NULL = zeros / not wanted).
 * Execution form, chosen per plan: equal-order cascades of state dimension <= 4 (one or two biquads, up to
 * four first-order sections, one section of order 3 or 4) run as ONE kernel that reads x once (chained scan with decoupled
 * look-back); other shapes as a block scan in three launches; cascades of mixed orders or beyond
 * those sizes as consecutive passes.  A plan owns scratch state for its launches: use one plan per
 * concurrent stream.  In place (out_dev == in_dev) is allowed in every form.
 * Non-finite input: a NaN or Inf in sample p of row r reaches out[r][p .. n) and all of zf[r], and no other row, in
 * every form: nothing from p on is ever finite again, however far behind the sample lies (a transition power that
 * has underflowed to zero times a non-finite state is NaN, not 0), everything before p and every other row are what
 * they are without it.  That is bit for bit in the three-launch form.  The single pass is reproducible to rounding
 * only, with or without a bad sample: a chunk's start state is a sum that closes on whichever earlier chunk of the
 * row has published its prefix when the wave looks, every choice the same sum in another association, so two applies
 * of one plan on one input may differ in the last bit (measured: one sample one ulp off in 18 of 150 applies).  A
 * look-back in double-double rounded once removes that and costs 7-8 % of the kernel (256 x 1e7 fp64, same box: 9.48
 * -> 10.21 ms two biquads, 10.84 -> 11.59 ms four first-order sections): not built in.
 * Such a NaN is data: wfk_iir_status stays WFK_OK and the plan keeps its form.
 * (+-Inf comes out as NaN in most places, as from scipy.signal.lfilter: non-finite is the promise, not the value.)
 * wfk_iir_apply() allocates nothing and does not synchronise: the single pass clears its tickets and chunk flags with
 * a small kernel in front of its own, a cut cascade repacks zi / zf with device-to-device copies.                  */
typedef struct wfk_iir_plan wfk_iir_plan;
int wfk_iir_plan_create(int32_t n_sections, const int32_t* orders, const double* b,
                        const double* a, int64_t n, int32_t batch,
                        int kind /* WFK_OUT_F64|F32 */, wfk_iir_plan** out);
int wfk_iir_state_dim(const wfk_iir_plan* plan);
int wfk_iir_apply(wfk_iir_plan* plan, const void* in_dev, int64_t in_stride, void* out_dev,
                  int64_t out_stride, const double* zi_dev, double* zf_dev, double initial,
                  void* hip_stream);
/* Synchronises `hip_stream`; WFK_ETIMEOUT if a single-pass launch of this plan since the last check ran
 * out of look-back polls (its outputs then hold NaN -- never silently: the same condition also fails the
 * NEXT wfk_iir_apply of the plan).  The plan switches to the three-launch form, so launching again works. */
int wfk_iir_status(wfk_iir_plan* plan, void* hip_stream);
/* What the next wfk_iir_apply launches, one entry per pass of a cut cascade, joined with " + ":
 * "iir_onepass<T,NSEC,ORD,PLAIN>" (" persistent" behind it when the grid is a bounded set of waves per row),
 * "iir_pass<T,NSEC,ORD>" for the three-launch form (0,0: the runtime-shaped build), "iir_scale<T>" for a pure gain,
 * "" for n == 0.  The apply and the name read one decision; once a look-back timeout has been reported the name is
 * that of the three-launch form.  The string belongs to the calling thread and lasts until its next call.         */
const char* wfk_iir_kernel_name(const wfk_iir_plan* plan);
int wfk_iir_plan_destroy(wfk_iir_plan* plan);

/* -- IIR stage with one cascade PER ROW ------------------------------------------------------- */
/* Row r runs through its OWN cascade: out[r] = F_r(in[r] - initial[r]) + initial[r] -- every flux line has its
 * own exp-decay correction (exp_decay_filter / predistort / distort, waveforms/distortion.py:100-185, 298-346).
 * The SHAPE (n_sections, orders) is shared by all rows; the coefficients are not: b_rows / a_rows hold, row after
 * row, the sections back to back with orders[s]+1 coefficients each, as wfk_iir_plan_create takes them for one row
 * (a[0] of a section need not be 1; a row with a lower order is padded with zero coefficients, which is exact for
 * this form).  zi_dev / zf_dev: optional [batch][state_dim] device arrays in scipy's layout per row; initial_dev:
 * optional [batch] device array (NULL = zeros).
 * Shapes: sections of EQUAL order >= 1 with a total state dimension <= 4 -- one section of order 1..4, 1..4
 * first-order sections, one or two biquads; anything else: WFK_EUNSUP, wfk_last_error() names the limit.
 * One kernel (iir_rows_tile): a workgroup owns a row and walks it tile by tile through LDS, x read once and y
 * written once; no workgroup waits for another, so there is no status call and no timeout, and results are
 * bitwise reproducible and independent of a row's position in the batch.  The plan holds one table of block
 * transition matrices per row (built in quad precision at creation, ~18 KB per row at state dimension 4) and no
 * scratch: a plan may serve several streams at once.  Non-finite input: a NaN or Inf in sample p of row r reaches
 * out[r][p .. n) and all of zf[r] (the entries of its own sections; padding entries stay zero), none of which is ever
 * finite, and no other row; out[r][0 .. p) and the other rows are bit for bit what they are without it.
 * wfk_iir_rows_apply() allocates nothing and does not
 * synchronise; in place (out_dev == in_dev) is allowed; strides are in elements.                              */
typedef struct wfk_iir_rows_plan wfk_iir_rows_plan;
int wfk_iir_rows_plan_create(int32_t n_sections, const int32_t* orders, const double* b_rows,
                             const double* a_rows, int64_t n, int32_t batch,
                             int kind /* WFK_OUT_F64|F32 */, wfk_iir_rows_plan** out);
int wfk_iir_rows_state_dim(const wfk_iir_rows_plan* plan);
int wfk_iir_rows_apply(wfk_iir_rows_plan* plan, const void* in_dev, int64_t in_stride, void* out_dev,
                       int64_t out_stride, const double* zi_dev, double* zf_dev,
                       const double* initial_dev, void* hip_stream);
/* The same launch with ONE input row for all rows: every row r reads in_dev[0..n) (row stride 0 inside) and
 * writes out[r] = F_r(in - initial[r]) + initial[r] -- one signal through `batch` candidate corrections, the
 * shape of a fit (phase_curve below).  `out` must not overlap `in` (WFK_EINVAL): rows are written while others
 * still read.  Otherwise as wfk_iir_rows_apply, whose own checks (in_stride >= n) are unchanged.              */
int wfk_iir_rows_apply_shared_in(wfk_iir_rows_plan* plan, const void* in_dev, void* out_dev, int64_t out_stride,
                                 const double* zi_dev, double* zf_dev, const double* initial_dev,
                                 void* hip_stream);
/* "iir_rows_tile<T,NSEC,ORD>"; the string lives as long as the plan */
const char* wfk_iir_rows_kernel_name(const wfk_iir_rows_plan* plan);
int wfk_iir_rows_plan_destroy(wfk_iir_rows_plan* plan);

/* -- sampler -> IIR (-> FIR) chain ------------------------------------------------------------ */
/* out = F(wav(t) - initial) + initial for every channel of `prog` on `grid`, F the cascade of wfk_iir_plan_create
 * (same section layout, same zi / zf state layout, [n_channels][state_dim]) -- Waveform.sample(filters=(sos, initial))
 * (waveforms/waveform.py:190-203, chunked with carried zi :244-251); with `ker_host` != NULL followed by the FIR of
 * wfk_fir_plan_create (ker_per_row != 0: kers_host[channel * K + k]) -- predistort(wav(t), filters, ker)
 * (waveforms/distortion.py:298-337).  Everything stays on the device.  When the program is fully fused (carrier-envelope
 * ops only, real amplitudes, no clip) and the cascade's first pass is in the single-pass form (state dimension <= 4),
 * the wave that owns a chunk of the scan (8192 or 16384 samples) EVALUATES its input instead of loading it (iir_sampled): the
 * unfiltered samples never touch HBM and the pass moves the 8 (4) B/sample of its output only.  Otherwise
 * sampler -> (in place) IIR.  The FIR stage reads the filtered rows from a workspace the plan owns.
 * Non-finite samples: a NaN or Inf that channel r's program evaluates to at sample p reaches out[r][p .. n) and zf[r]
 * as through wfk_iir_apply (with a FIR behind the cascade: from p - K/2 on, back to the start of the first window that
 * reads sample p at most), and no other row; it is data, not a time-out: the status stays WFK_OK.
 * wfk_chain_iir_launch() allocates nothing and does not synchronise; status / timeout semantics as wfk_iir_status
 * (after a timeout the plan runs unfused in the three-launch form).                                            */
typedef struct wfk_chain_iir_plan wfk_chain_iir_plan;
int wfk_chain_iir_plan_create(const wfk_program* prog, const wfk_grid* grid, int32_t n_sections,
                              const int32_t* orders, const double* b, const double* a,
                              const double* ker_host /* or NULL */, int32_t K, int32_t ker_per_row,
                              int kind /* WFK_OUT_F64|F32 */, wfk_chain_iir_plan** out);
int wfk_chain_iir_is_fused(const wfk_chain_iir_plan* plan);
const char* wfk_chain_iir_unfused_reason(const wfk_chain_iir_plan* plan);
/* "iir_sampled<T,NSEC,ORD,PLAIN>" (+ later passes / FIR) or the kernels of the unfused path */
const char* wfk_chain_iir_kernel_name(const wfk_chain_iir_plan* plan);
int64_t wfk_chain_iir_table_bytes(const wfk_chain_iir_plan* plan);
int wfk_chain_iir_state_dim(const wfk_chain_iir_plan* plan);
int wfk_chain_iir_launch(wfk_chain_iir_plan* plan, void* out_dev, int64_t out_stride, const double* zi_dev,
                         double* zf_dev, double initial, void* hip_stream);
int wfk_chain_iir_status(wfk_chain_iir_plan* plan, void* hip_stream);
int wfk_chain_iir_plan_destroy(wfk_chain_iir_plan* plan);

/* ---- sampler -> per-row IIR chain: every row its own waveform AND its own cascade ------------------------------
 * predistort(wav(t), filters=[exp_decay_filter(...), ...], initial=level) per flux line (reference
 * waveforms/distortion.py:100-185, :298-321), device-resident:  out[c] = F_c(wav_c(t) - initial[c]) + initial[c] for
 * the channels c of `prog` on `grid`.  The batch is the program's channel count; coefficient layout (b_rows / a_rows:
 * n_channels rows of the sections back to back, each orders[s] + 1 long), the shape limits, zi / zf / initial_dev
 * are those of wfk_iir_rows_plan_create / wfk_iir_rows_apply.
 * Fused, ONE kernel: the workgroup that owns a row evaluates each tile of 4096 samples into LDS and filters it there
 * -- "iir_rows_sampled<T,NSEC,ORD>" on fine grids (fully fused real channels without clip whose parameter blocks
 * fit 2048 doubles of LDS: stride-256 chains), "iir_rows_short<T,NSEC,ORD>" at AWG sample rates (a pure short-tier
 * plan of real channels: runs of one piece).  The unfiltered samples never touch HBM, the launch moves the 8 (4)
 * B/sample of its output, and rows of any length fuse.  Everything else -- complex channels, generic terms, clip on a
 * fine grid, table / mollifier envelopes and corrected carriers at AWG rates, mixed plans, WFK_CHAIN_UNFUSED=1 --
 * runs the sampler into `out` and iir_rows_tile in place on it; the name is then the two kernels joined with " + "
 * and the reason is never empty.  The decision is taken once, at creation.
 * Non-finite samples: a NaN or Inf that channel c's program evaluates to at sample p reaches out[c][p .. n) and
 * zf[c], as through wfk_iir_rows_apply, and no other row.
 * wfk_chain_iir_rows_launch() allocates nothing and does not synchronise; n == 0 launches nothing.  The strings
 * live as long as the plan.                                                                                      */
typedef struct wfk_chain_iir_rows_plan wfk_chain_iir_rows_plan;
int wfk_chain_iir_rows_plan_create(const wfk_program* prog, const wfk_grid* grid, int32_t n_sections,
                                   const int32_t* orders, const double* b_rows, const double* a_rows,
                                   int kind /* WFK_OUT_F64|F32 */, wfk_chain_iir_rows_plan** out);
int wfk_chain_iir_rows_is_fused(const wfk_chain_iir_rows_plan* plan);
const char* wfk_chain_iir_rows_unfused_reason(const wfk_chain_iir_rows_plan* plan);
const char* wfk_chain_iir_rows_kernel_name(const wfk_chain_iir_rows_plan* plan);
int64_t wfk_chain_iir_rows_table_bytes(const wfk_chain_iir_rows_plan* plan);
int wfk_chain_iir_rows_state_dim(const wfk_chain_iir_rows_plan* plan);
int wfk_chain_iir_rows_launch(wfk_chain_iir_rows_plan* plan, void* out_dev, int64_t out_stride, const double* zi_dev,
                              double* zf_dev, const double* initial_dev, void* hip_stream);
int wfk_chain_iir_rows_plan_destroy(wfk_chain_iir_rows_plan* plan);

/* -- whole-signal transfer function ------------------- */
/* out = irfft(rfft(in) * H) per row; rows contiguous (stride n); H_dev = n/2+1 complex128
 * bins on the device (f_k = k*fs/n).  Replaces the scipy.fftpack calls of
 * reflection / correct_reflection (waveforms/distortion.py:208-223).                  */
typedef struct wfk_spectral_plan wfk_spectral_plan;
int wfk_spectral_plan_create(int64_t n, int32_t batch, int kind, wfk_spectral_plan** out);
/* The one H serves all `batch` rows.  In place (out_dev == in_dev) is allowed: the input is copied to a
 * staging buffer of the plan before anything is written.  Non-finite input: a NaN or Inf anywhere in row r reaches
 * all of out[r] (one transform per row: no element of it is finite) and no other row -- the batched transform never
 * mixes rows; the other rows are bit for bit what they are without it.  Asynchronous on `hip_stream`:
 * wfk_spectral_apply() allocates nothing and does not synchronise (the plan owns rocFFT's work buffer).  */
int wfk_spectral_apply(wfk_spectral_plan* plan, const void* in_dev, void* out_dev,
                       const void* H_dev, void* hip_stream);
int wfk_spectral_plan_destroy(wfk_spectral_plan* plan);

/* -- per-row reflection / inverse reflection / delay, transfer function built on the device --- */
/* out[r] = irfft(rfft(in[r]) * H_r) for `batch` rows of n samples, H_r(k) the product of row r's terms at
 * f_k = k * sample_rate / n; with e = exp(-2 pi i f_k tau):
 *   WFK_SPEC_REFLECT  (1 - A) / (1 - A e)   reflection(sig, A, tau, fs)          (waveforms/distortion.py:188-210)
 *   WFK_SPEC_CORRECT  (1 - A e) / (1 - A)   correct_reflection(sig, A, tau, fs)  (waveforms/distortion.py:213-223)
 *   WFK_SPEC_DELAY    e                     band-limited circular delay by tau (A ignored, tau of either sign)
 * terms_host: the rows' terms back to back in row order, n_terms_per_row_host[r] of them for row r (0 ..
 * WFK_SPEC_ROWS_MAX_TERMS; 0: the row passes unchanged).  More terms, an unknown kind, a tau that is not finite,
 * or |A| >= 1 on a REFLECT / CORRECT term (the reference divides by zero at A = 1): WFK_EINVAL.
 * H is not stored: one kernel (spec_rows_mul) makes one pass over the R2C output and forms H per (row, bin) from
 * the row's terms; the phase k * (tau fs / n) is reduced to [-1/2, 1/2] cycles BEFORE it is rounded (the plan
 * keeps tau fs / n as a quad-precision (hi, lo) pair), so delays of thousands of cycles cost no accuracy.
 * The plan owns the batched rocFFT pair, its work / spectrum / staging buffers and the term table.
 * wfk_spectral_rows_apply() allocates nothing and does not synchronise; strides are in elements, >= n, otherwise
 * arbitrary; in place (out_dev == in_dev) and any other overlap are allowed (the input is staged before anything
 * is written).  A row's result does not depend on its position in the batch.  One plan per concurrent stream.
 * Non-finite input: a NaN or Inf anywhere in row r reaches all of out[r] (one transform per row: no element of it is
 * finite) and no other row; the other rows are bit for bit what they are without it.                            */
#define WFK_SPEC_ROWS_MAX_TERMS 8
enum { WFK_SPEC_REFLECT = 0, WFK_SPEC_CORRECT = 1, WFK_SPEC_DELAY = 2 };
typedef struct wfk_spec_term {
  int32_t kind;      /* WFK_SPEC_* */
  int32_t reserved;  /* 0 */
  double A;
  double tau;        /* seconds */
} wfk_spec_term;
typedef struct wfk_spectral_rows_plan wfk_spectral_rows_plan;
int wfk_spectral_rows_plan_create(int64_t n, int32_t batch, int kind /* WFK_OUT_F64|F32 */, double sample_rate,
                                  const wfk_spec_term* terms_host, const int32_t* n_terms_per_row_host,
                                  wfk_spectral_rows_plan** out);
int wfk_spectral_rows_apply(wfk_spectral_rows_plan* plan, const void* in_dev, int64_t in_stride, void* out_dev,
                            int64_t out_stride, void* hip_stream);
int wfk_spectral_rows_plan_destroy(wfk_spectral_rows_plan* plan);
/* host only, no device: tau * sample_rate / n in quad precision as the (hi, lo) pair of doubles the plan stores */
int wfk_spectral_rows_phase_step(double tau, double sample_rate, int64_t n, double* hi_out, double* lo_out);

/* -- per-row shift: the reference's delay in time, one skew per row ----------------------------- */
/* out[r] = shift(in[r], delay_r, dt) (waveforms/distortion.py:12-39) for `batch` rows of n samples.  The caller
 * splits every delay with the reference's own expressions, points = int(delay // dt), delta = delay / dt - points
 * (delta in [0, 1]: Python's floor division makes 1.0 // 0.1 = 9 and delta = 1, which is legal), and the device
 * computes, with x[k] = 0 for k < 0,
 *   s[j] = (1 - delta) x[j] + delta x[j - 1]  if delta > 0,   s[j] = x[j] otherwise (a copy, bit for bit),
 *   y[i] = s[i - points] if 0 <= i - points < n, 0 otherwise
 * -- linear interpolation and ZERO fill at both ends (not the circular, band-limited WFK_SPEC_DELAY above); rows
 * with |points| >= n come out all zero.  Unlike the reference, rows keep n samples for n < 3, and the zero tap on
 * x[j + 1] is not multiplied (an inf there does not make sample j NaN).  points_host / delta_host: `batch` entries.
 * n < 0, batch < 1, a delta outside [0, 1] or not finite, a kind other than F64 / F32, null pointers: WFK_EINVAL;
 * no device: WFK_EHIP.  One kernel (shift_rows<T>), one read and one write per sample, float rows computed in
 * double and rounded once; the plan owns the small row table and nothing else, so it may serve several streams.
 * wfk_shift_rows_apply() allocates nothing and does not synchronise; strides are in elements, >= n.  OUT OF PLACE
 * only: if [in, in + (batch - 1) * in_stride + n) overlaps the same range of out, WFK_EINVAL.  n = 0: no-op.   */
typedef struct wfk_shift_rows_plan wfk_shift_rows_plan;
int wfk_shift_rows_plan_create(int64_t n, int32_t batch, int kind /* WFK_OUT_F64|F32 */, const int64_t* points_host,
                               const double* delta_host, wfk_shift_rows_plan** out);
int wfk_shift_rows_apply(wfk_shift_rows_plan* plan, const void* in_dev, int64_t in_stride, void* out_dev,
                         int64_t out_stride, void* hip_stream);
/* "shift_rows<double>" or "shift_rows<float>"; a static string */
const char* wfk_shift_rows_kernel_name(const wfk_shift_rows_plan* plan);
int wfk_shift_rows_plan_destroy(wfk_shift_rows_plan* plan);

/* -- per-row DAC codes: scale, round and saturate rows to int16 ---------------------------------- */
/* `batch` real rows of n samples (kind: WFK_OUT_F64 or WFK_OUT_F32, the INPUT rows) become int16 DAC codes.  Input
 * row r has gain_host[r] (LSB per unit of the signal) and offset_host[r] (LSB), both finite.  Per sample, in double
 * (a float sample is widened first) and without a fused multiply-add,
 *   v = fl(fl(x * gain) + offset),   q = rint(v) (half to even),   lo = -2^(bits - 1),   hi = 2^(bits - 1) - 1,
 *   c = 0 if v is NaN (counted as nan), lo if q < lo (below; -inf too), hi if q > hi (above; +inf too), q otherwise,
 *   word = c * 2^shift as int16   (2 <= bits <= 16, 0 <= shift <= 16 - bits: the low `shift` bits are zero).
 * interleave = k in {1, 2}, batch a multiple of k: output row g holds the input rows g k .. g k + k - 1 sample by
 * sample, out[g, i k + j] = word[g k + j, i] (k = 2: rows [I, Q] become I0 Q0 I1 Q1 ...); there are batch / k output
 * rows of k n codes.  n < 0, batch < 1, a gain or offset that is not finite (the row is named), bits / shift /
 * interleave out of range, a batch that is no multiple of the interleave, a kind other than F64 / F32, null
 * pointers, more than 2^31 - 1 workgroups: WFK_EINVAL, before any device work; no device: WFK_EHIP.
 * wfk_dac_rows_apply() allocates nothing and does not synchronise.  in_stride is in samples, >= n; out_stride in
 * codes, >= k n where there is more than one output row.  counts_dev: NULL, or batch * 3 int64 on the device,
 * [below, above, nan] per INPUT row; every apply OVERWRITES them (zeroed on the stream, then added to with integer
 * atomics: bitwise reproducible); without them the kernel does no counting.  OUT OF PLACE only, and the input is
 * never written: an output extent that meets the input extent, or counts that meet either, WFK_EINVAL.  n = 0:
 * a no-op that still zeroes the counts.  The plan owns the small row table and nothing else, so it may serve
 * several streams. */
typedef struct wfk_dac_rows_plan wfk_dac_rows_plan;
int wfk_dac_rows_plan_create(int64_t n, int32_t batch, int kind /* WFK_OUT_F64|F32: the INPUT rows */,
                             const double* gain_host, const double* offset_host, int bits, int shift,
                             int interleave, wfk_dac_rows_plan** out);
int wfk_dac_rows_apply(wfk_dac_rows_plan* plan, const void* in_dev, int64_t in_stride,
                       int16_t* out_dev, int64_t out_stride /* in codes, >= interleave * n */,
                       int64_t* counts_dev /* batch * 3, or NULL */, void* hip_stream);
/* "dac_rows<double>" / "dac_rows<float>", or with counts "dac_rows_count<double>" / "dac_rows_count<float>" (the
 * interleave is an argument of the kernel, not part of its name); a static string */
const char* wfk_dac_rows_kernel_name(const wfk_dac_rows_plan* plan, int with_counts);
int wfk_dac_rows_plan_destroy(wfk_dac_rows_plan* plan);

/* -- sampler -> DAC codes: the AWG-rate sampler writes the int16 codes itself ---------------------- */
/* codes = wfk_dac_rows(wfk_plan_launch(prog on grid, WFK_OUT_F64)) for the channels of `prog`, bit for bit -- codes and
 * counts -- without the float64 rows: gain_host / offset_host hold one value per channel, bits / shift / interleave
 * and the formula are those of wfk_dac_rows_plan_create, whose argument checks run first, before any device work;
 * complex channels: WFK_EINVAL.  Fused -- the sampler plan is a pure short-tier plan (no time list, not mixed, no
 * second launch of the general kernel) and interleave == 1 -- ONE kernel, "wfk_sample_short_dac<16,FAM,COUNT>": the
 * short tier's unit pipeline with the scaling, rounding and saturation behind each sample, 2 B per sample stored.
 * Everything else -- WFK_CHAIN_UNFUSED=1, n == 0, no short plan, a mixed plan, interleave == 2 -- runs the sampler
 * into scratch_dev (n_channels float64 rows, scratch_stride >= n samples apart) and dac_rows on it; the name is
 * then the kernels joined with " + " and the reason is never empty.  The decision is taken once, at creation.
 * wfk_chain_dac_launch() enqueues its kernels (the zeroing of the counts among them) on `hip_stream`, and that is all
 * it does to the device (as wfk_avg_apply: it may be called while the stream is being captured).  out_dev:
 * n_channels / interleave rows of interleave * n codes, out_stride codes apart (a lone row's stride is not read),
 * aligned to 2 bytes, anywhere in a wider buffer; counts_dev: NULL, or n_channels * 3 int64 [below, above, nan],
 * OVERWRITTEN by every launch, meeting neither the codes nor the scratch; scratch_dev: NULL for a fused plan (not
 * touched), WFK_EINVAL for an unfused one.  n == 0 launches no sampler and still zeroes the counts.  The strings live
 * as long as the plan; one plan per concurrent stream. */
typedef struct wfk_chain_dac_plan wfk_chain_dac_plan;
int wfk_chain_dac_plan_create(const wfk_program* prog, const wfk_grid* grid, const double* gain_host,
                              const double* offset_host, int bits, int shift, int interleave,
                              wfk_chain_dac_plan** out);
int wfk_chain_dac_is_fused(const wfk_chain_dac_plan* plan);
const char* wfk_chain_dac_unfused_reason(const wfk_chain_dac_plan* plan);
const char* wfk_chain_dac_kernel_name(const wfk_chain_dac_plan* plan, int with_counts);
int64_t wfk_chain_dac_table_bytes(const wfk_chain_dac_plan* plan);
int wfk_chain_dac_launch(wfk_chain_dac_plan* plan, int16_t* out_dev, int64_t out_stride,
                         int64_t* counts_dev /* n_channels * 3, or NULL */, void* scratch_dev /* or NULL */,
                         int64_t scratch_stride, void* hip_stream);
int wfk_chain_dac_plan_destroy(wfk_chain_dac_plan* plan);

/* -- per-row gate markers: widened, as bytes or into one bit of the DAC codes -------------------- */
/* `batch` real rows of n samples (kind: WFK_OUT_F64 or WFK_OUT_F32) drive batch / group marker rows: the marker
 * line that opens a switch or blanks an amplifier around every pulse, derived from the IDEAL gate rows (exact zeros
 * outside the pulses), not from predistorted ones.  group = k in {1, 2}, batch a multiple of k: marker row g is driven
 * by the input rows g k .. g k + k - 1 (k = 2: the I and Q of a pair, as wfk_dac_rows pairs them).  Marker row g has
 * threshold_host[g] (finite, >= 0) and lead_host[g], trail_host[g] (samples, in [0, WFK_MARKER_MAX_EDGE]).  Exact,
 * in integers:
 *   active[g, i] = any_j  fabs((double)x[g k + j, i]) > threshold[g]   (NaN is inactive, +-inf active, -0.0 and a
 *                                                                       sample equal to the threshold inactive)
 *   m[g, i]      = any    active[g, j]  for j in [i - trail[g], i + lead[g]], clipped to [0, n)
 * so the marker rises `lead` samples before the first active sample of a burst and falls `trail` samples after the
 * last, and gaps shorter than lead + trail + 1 close.  Two forms:
 *   wfk_marker_rows_apply():        out[g, i] = m[g, i] as uint8 0 / 1, batch / k rows of n bytes;
 *   wfk_marker_rows_apply_codes():  codes is batch / k rows of k n int16 in the layout wfk_dac_rows(interleave = k)
 *     produces, and codes[g, p] = (codes[g, p] & ~(1 << bit)) | (m[g, p / k] << bit), 0 <= bit <= 15, IN PLACE: the
 *     bit is overwritten, not OR-ed (a second apply gives the same codes), and no other bit of a code changes.
 * n < 0, batch < 1, a group other than 1 or 2, a batch that is no multiple of it, a threshold that is negative or
 * not finite, a lead or trail that is negative or exceeds WFK_MARKER_MAX_EDGE (the row is named: "row 3: lead exceeds
 * 4096"), a kind other than F64 / F32, null pointers, more than 2^31 - 1 workgroups: WFK_EINVAL, before any device
 * work; no device: WFK_EHIP.
 * wfk_marker_rows_apply() and wfk_marker_rows_apply_codes() allocate nothing and do not synchronise.
 * in_stride is in samples, >= n; out_stride in bytes, >= n,
 * codes_stride in codes, >= k n, where there is more than one marker row.  counts_dev: NULL, or batch / k * 2 int64
 * on the device, [high, pulses] per marker row -- the samples with m = 1, and those of them with i = 0 or
 * m[g, i - 1] = 0; every apply OVERWRITES them (zeroed on the stream, then added to with integer atomics: bitwise
 * reproducible); without them the kernel does no counting.  The input is never written; out / codes may share no
 * memory with it, counts with neither; a bit outside [0, 15], rows not aligned to their element, a stride below
 * the row: WFK_EINVAL.  n = 0: a no-op that still zeroes the counts.  The plan owns the small row table and nothing
 * else, so it may serve several streams. */
#define WFK_MARKER_MAX_EDGE 4096   /* 2 us at 2 GS/s */
typedef struct wfk_marker_rows_plan wfk_marker_rows_plan;
int wfk_marker_rows_plan_create(int64_t n, int32_t batch, int kind /* WFK_OUT_F64|F32 */, int group,
                                const double* threshold_host, const int32_t* lead_host,
                                const int32_t* trail_host /* batch / group of each */, wfk_marker_rows_plan** out);
int wfk_marker_rows_apply(wfk_marker_rows_plan* plan, const void* in_dev, int64_t in_stride,
                          uint8_t* out_dev, int64_t out_stride /* in bytes, >= n */,
                          int64_t* counts_dev /* batch / group * 2, or NULL */, void* hip_stream);
int wfk_marker_rows_apply_codes(wfk_marker_rows_plan* plan, const void* in_dev, int64_t in_stride,
                                int16_t* codes_dev, int64_t codes_stride /* in codes, >= group * n */, int bit,
                                int64_t* counts_dev /* batch / group * 2, or NULL */, void* hip_stream);
/* the samples one workgroup covers: 16384 as bytes, 8192 / group into codes (0 for a null plan) */
int64_t wfk_marker_rows_span(const wfk_marker_rows_plan* plan, int into_codes);
/* "marker_rows<double>", "marker_rows_codes<double>", with counts "marker_rows_count<double>",
 * "marker_rows_codes_count<double>", and the same four with <float> (the group is an argument of the kernel, not
 * part of its name); a static string */
const char* wfk_marker_rows_kernel_name(const wfk_marker_rows_plan* plan, int into_codes, int with_counts);
int wfk_marker_rows_plan_destroy(wfk_marker_rows_plan* plan);

/* -- cutting code rows at their marker: a segment table and the kept codes, packed ---------------- */
/* `rows` rows of n samples, width = k in {1, 2} int16 codes per sample (k = 2: the interleaved layout of
 * wfk_dac_rows(interleave = 2) and wfk_marker_rows(group = 2)), are cut where their marker is low, so that only the
 * stretches around the pulses are sent on.  The mask m[g, i] is, per apply,
 *   wfk_segment_rows_apply_bit():    any_j ((codes[g, i k + j] >> bit) & 1), 0 <= bit <= 15 -- the codes alone;
 *   wfk_segment_rows_apply_marks():  marks[g, i] != 0, rows of n bytes as wfk_marker_rows_apply() writes them.
 * align = A, a power of two in [1, WFK_SEGMENT_MAX_ALIGN], is the instrument's granularity: with Q = ceil(n / A),
 * granule q is kept when any m[g, i], i in [q A, min((q + 1) A, n)), is set, and the segments of a row are the maximal
 * runs [q0, q1) of kept granules, in ascending order, j = 0 .. count - 1:
 *   start_j = q0 A,   length_j = min(q1 A, n) - start_j,   offset_j = length_0 + ... + length_(j-1),   kept = all of them.
 * Every start and offset is a multiple of A, every length but possibly a row's last.  Outputs, all the caller's,
 * their sizes fixed at plan creation:
 *   table  rows of 3 max_segments int32: entry j < min(count, max_segments) is [start_j, length_j, offset_j]; no
 *          other entry is touched;
 *   packed rows of k capacity int16: for p < min(kept, capacity) the k codes of the p-th kept sample, verbatim (the
 *          marker bit with them); nothing else is touched.  The cut at `capacity` is by position alone, independent of
 *          the table's; a segment that straddles it is written up to it;
 *   used   rows * 2 int64, [count, kept] per row: the TRUE totals whatever was cut, overwritten by every apply
 *          (written by the kernel that owns the row: no atomics, no zeroing).  Required.
 * The caller compares used with max_segments and capacity.  table = packed = NULL is the sizing pass: only used is
 * written.  A side that holds nothing (max_segments = 0, capacity = 0) is not looked at and may be NULL next to the
 * other.  n = 0 zeroes used and does nothing else.  codes and marks are never written.  The result is a pure function
 * of the inputs: two applies agree to the bit.
 * n < 0 or n > 2^31 - 1, rows < 1, a width other than 1 or 2, an align that is no power of two in [1, 4096],
 * max_segments < 0, capacity < 0 or > n, more than 2^31 - 1 workgroups: WFK_EINVAL with the argument named, before any
 * device work; no device: WFK_EHIP.
 * wfk_segment_rows_apply_bit() and wfk_segment_rows_apply_marks() enqueue their three kernels (two in the sizing pass;
 * for n = 0 the zeroing of used alone) on `hip_stream`, and that is all they do to the device (as wfk_avg_apply: they
 * may be called while the stream is being captured; a replay reads the codes and marks anew and overwrites used).
 * Strides are in elements of their side and, where there is more than one row, at least the row: codes_stride >= k n,
 * marks_stride >= n, table_stride >= 3 max_segments (int32), packed_stride >= k capacity.  Every side is aligned to its
 * element, no output meets an input or another output, used (8-byte aligned) meets none of them; a bit outside
 * [0, 15], a NULL table with a packed buffer or the reverse, a NULL used: WFK_EINVAL.
 * The plan owns a workspace of rows x blocks x 4 int64 that the three launches of an apply hand to each other, so a
 * plan serves ONE STREAM AT A TIME (and one graph at a time). */
#define WFK_SEGMENT_MAX_ALIGN 4096
typedef struct wfk_segment_rows_plan wfk_segment_rows_plan;
int wfk_segment_rows_plan_create(int64_t n, int32_t rows, int width, int64_t align, int64_t max_segments,
                                 int64_t capacity, wfk_segment_rows_plan** out);
int wfk_segment_rows_apply_bit(wfk_segment_rows_plan* plan, const int16_t* codes_dev, int64_t codes_stride, int bit,
                               int32_t* table_dev, int64_t table_stride, int16_t* packed_dev, int64_t packed_stride,
                               int64_t* used_dev /* rows * 2 */, void* hip_stream);
int wfk_segment_rows_apply_marks(wfk_segment_rows_plan* plan, const int16_t* codes_dev, int64_t codes_stride,
                                 const uint8_t* marks_dev, int64_t marks_stride, int32_t* table_dev,
                                 int64_t table_stride, int16_t* packed_dev, int64_t packed_stride,
                                 int64_t* used_dev /* rows * 2 */, void* hip_stream);
/* the samples one workgroup covers: max(8192, 64 align) (0 for a null plan) */
int64_t wfk_segment_rows_span(const wfk_segment_rows_plan* plan);
/* launch 0, 1, 2: "segment_count<1, false>", "segment_scan", "segment_pack<1, false>" -- <width, marks form>; a
 * static string ("" for another launch or a null plan) */
const char* wfk_segment_rows_kernel_name(const wfk_segment_rows_plan* plan, int launch, int with_marks);
int wfk_segment_rows_plan_destroy(wfk_segment_rows_plan* plan);

/* -- the waveform library of a segment table: equal segments of a row share one slot -------------- */
/* A gate sequence plays the same few pulses many times per channel, and the packed side of wfk_segment_rows holds each
 * of them again.  The library keeps one copy per row of every distinct segment.  The plan is made for `rows` rows,
 * width = k in {1, 2}, max_segments and capacity (those of the wfk_segment_rows plan whose outputs it reads) and
 * lib_capacity in [0, capacity].  Inputs per apply, device memory, never written, as wfk_segment_rows wrote them:
 *   table   rows of 3 max_segments int32;   packed  rows of k capacity int16;   used  rows * 2 int64 [count, kept].
 * Two segments of a row are EQUAL when their lengths are equal and their k length codes are equal verbatim, marker bits
 * included.  Among equal segments the one with the lowest j is the FIRST.  The firsts, in ascending j, are the row's
 * slots u = 0, 1, ...:
 *   lib_offset_u = length of slot 0 + ... + length of slot u - 1,   unique = the number of slots,
 *   lib_kept = the lengths of all slots.
 * Outputs, all the caller's; each of the first three is optional, NULL: not written:
 *   plays    rows of 3 max_segments int32: entry j < count is [start_j, length_j, lib_offset of the slot of j]; no
 *            other entry is touched.  The layout of table: (plays, library) expand as (table, packed) do;
 *   slots    rows of max_segments int32: entry j < count is the slot u of segment j; no other entry is touched;
 *   library  rows of k lib_capacity int16: the codes of slot u lie at k lib_offset_u, verbatim, for the samples
 *            p < min(lib_kept, lib_capacity); nothing else is touched.  The cut at `lib_capacity` is by position, as
 *            for packed; plays holds the true offsets whatever the cut;
 *   lib_used rows * 2 int64, [unique, lib_kept] per row: the TRUE totals, overwritten by every apply (written by the
 *            kernel that owns the row: no atomics onto it, no zeroing).  Required.
 * plays = slots = library = NULL is the sizing pass: only lib_used is written.  A side that holds nothing
 * (max_segments = 0, capacity = 0, lib_capacity = 0) is not looked at and may be NULL.
 * A ROW THAT CANNOT BE READ is reported, not trusted: used[row] with count < 0, count > max_segments, kept < 0 or
 * kept > capacity, or an entry j < count with length <= 0, offset < 0 or offset + length > capacity (formed in 64
 * bits).  Such a row gets lib_used[row] = [-1, -1] and nothing else of it is written; the other rows are unaffected.
 * No content of table / packed / used makes a kernel read or write outside the sides it was given.  (In a row that the
 * segment stage wrote, lib_kept <= kept; where the entries of a row overlap each other, the third column of plays is
 * lib_offset modulo 2^32.)  Every output is a pure function of the inputs: two applies agree to the bit, whatever
 * the order in which segments met in the kernels.
 * rows < 1, a width other than 1 or 2, max_segments < 0 or > 2^30, capacity < 0 or > 2^31 - 1, lib_capacity outside
 * [0, capacity], more than 2^31 - 1 workgroups: WFK_EINVAL with the argument named, before any device work; no device:
 * WFK_EHIP.
 * wfk_segment_library_apply() enqueues its four kernels (three in the sizing pass; with max_segments = 0 the one that
 * writes lib_used alone) on `hip_stream`, and that is all it does to the device (as wfk_avg_apply: it may be called
 * while the stream is being captured; a replay reads table, packed and used anew and overwrites lib_used).
 * Strides are in elements of their side and, where there is more than one row, at least the row: table_stride and
 * plays_stride >= 3 max_segments, slots_stride >= max_segments (int32), packed_stride >= k capacity, library_stride >=
 * k lib_capacity.  Every side is aligned to its element, no output meets an input or another output, lib_used (8-byte
 * aligned) meets none of them; a NULL used or lib_used: WFK_EINVAL.
 * The plan owns a workspace (a hash, a slot and two sums per segment, a hash table of the power of two >= 2
 * max_segments ids per row) that the launches of an apply hand to each other and that an apply rewrites before it
 * reads it, so a plan serves ONE STREAM AT A TIME (and one graph at a time).
 * The environment's WFK_SEGLIB_HASH_BITS = b, 0 <= b <= 64, read when the plan is made, keeps only the low b bits of
 * every hash: more segments meet in the table, and no result changes.  A value that is no whole number in [0, 64]
 * is ignored, as an unknown WFK_STATES_COUNTERS is: the plan keeps the full hash, and its kernel names show that. */
typedef struct wfk_segment_library_plan wfk_segment_library_plan;
int wfk_segment_library_plan_create(int32_t rows, int width, int64_t max_segments, int64_t capacity,
                                    int64_t lib_capacity, wfk_segment_library_plan** out);
int wfk_segment_library_apply(wfk_segment_library_plan* plan, const int32_t* table_dev, int64_t table_stride,
                              const int16_t* packed_dev, int64_t packed_stride, const int64_t* used_dev /* rows * 2 */,
                              int32_t* plays_dev /* or NULL */, int64_t plays_stride, int32_t* slots_dev /* or NULL */,
                              int64_t slots_stride, int16_t* library_dev /* or NULL */, int64_t library_stride,
                              int64_t* lib_used_dev /* rows * 2 */, void* hip_stream);
/* launch 0 .. 3: "seglib_hash", "seglib_match", "seglib_scan", "seglib_copy"; where WFK_SEGLIB_HASH_BITS cut the hash,
 * the first two end in " [hash bits b]".  The string lives as long as the plan ("" for another launch or a null
 * plan) */
const char* wfk_segment_library_kernel_name(const wfk_segment_library_plan* plan, int launch);
int wfk_segment_library_plan_destroy(wfk_segment_library_plan* plan);

/* -- playing a segment table back: table + waveform memory -> code rows, compared on the way ------ */
/* The inverse of the cut, on the device: what a sequencer plays from a table and a waveform memory, as dense rows, with
 * an optional comparison against the rows the table was cut from.  The plan is made for `rows` rows of n samples,
 * width = k in {1, 2} codes per sample, max_segments and capacity (the room of a packed / library row, in samples).
 * Inputs per apply, device memory, never written:
 *   table   rows of 3 max_segments int32 [start, length, offset], as wfk_segment_rows writes table or
 *           wfk_segment_library writes plays, or as the caller wrote it;
 *   packed  rows of k capacity int16: the packed side of wfk_segment_rows, or a library;
 *   used    rows * 2 int64, of which only the first of a row (count) is read;
 *   idle0, idle1  the idle code of each code of a sample (k = 1: idle0 alone), passed BY VALUE per apply: a captured
 *           graph replays the captured values;
 *   expect  rows of k n int16, or NULL: the rows the table was cut from.
 * A row is GOOD when 0 <= count <= max_segments, every entry j < count has length > 0, start >= 0, start + length <= n,
 * offset >= 0 and offset + length <= capacity (formed in 64 bits), and every entry 1 <= j < count has start_j >=
 * start_(j-1) + length_(j-1): ascending and disjoint (touching is good).  Everything the two stages write is good; a row
 * whose table overflowed max_segments is bad, as is a library cut at lib_capacity, whose offsets point past the room.
 * This is NARROWER than expand_segments of the Python package, which takes empty and overlapping entries (the later
 * one wins).  Outputs:
 *   out     rows of k n int16, or NULL.  For a good row, sample i holds the k codes at k (offset_j + i - start_j) of
 *           packed where start_j <= i < start_j + length_j, and (idle0, idle1) elsewhere -- by code index in the row,
 *           wherever the row starts.  All k n codes of a good row are written and nothing else: no gap of a strided
 *           row, nothing of a bad row;
 *   report  rows * 4 int64, [played, differ, stray, first] per row, required, overwritten by every apply:
 *           played = the lengths of the row's entries; differ = the samples inside a play where any of the k codes
 *           differs from expect; stray = the samples outside every play where any code of expect differs from its
 *           idle; first = the lowest sample counted by either, or -1.  Without expect: [played, 0, 0, -1].  A bad row:
 *           [-1, -1, -1, -1], and the other rows are unaffected.
 * out = NULL with expect is the verifying pass, out = expect = NULL the checking pass: only the report is written.
 * n = 0 writes the report and nothing else.  No content of table / packed / used makes a kernel read or write outside
 * the sides it was given.  Every output is a pure function of the inputs: two applies agree to the bit (the counts are
 * integer sums and a minimum, whatever the order in which workgroups arrive).
 * n outside [0, 2^31 - 1], rows < 1, a width other than 1 or 2, max_segments < 0 or > 2^30, capacity < 0 or > 2^31 - 1,
 * more than 2^31 - 1 workgroups: WFK_EINVAL with the argument named, before any device work; no device: WFK_EHIP.
 * wfk_segment_play_apply() enqueues its two kernels (one in the checking pass and for n = 0) on `hip_stream`, and that
 * is all it does to the device (as wfk_avg_apply: it may be called while the stream is being captured; a replay reads
 * table, packed, used and expect anew and overwrites the report).
 * Strides are in elements of their side and, where there is more than one row, at least the row: table_stride >= 3
 * max_segments (int32), packed_stride >= k capacity, out_stride and expect_stride >= k n.  Every side is aligned to its
 * element, out meets no input (expect among them), report (8-byte aligned) meets none of them; a side that holds
 * nothing (max_segments = 0, capacity = 0; n = 0 for out and expect) is not looked at; a NULL used or report:
 * WFK_EINVAL.
 * The plan owns a workspace of `rows` ints (the verdicts) that the first launch hands to the second, so a plan serves
 * ONE STREAM AT A TIME (and one graph at a time). */
typedef struct wfk_segment_play_plan wfk_segment_play_plan;
int wfk_segment_play_plan_create(int64_t n, int32_t rows, int width, int64_t max_segments, int64_t capacity,
                                 wfk_segment_play_plan** out);
int wfk_segment_play_apply(wfk_segment_play_plan* plan, const int32_t* table_dev, int64_t table_stride,
                           const int16_t* packed_dev, int64_t packed_stride, const int64_t* used_dev /* rows * 2 */,
                           int16_t idle0, int16_t idle1, int16_t* out_dev /* or NULL */, int64_t out_stride,
                           const int16_t* expect_dev /* or NULL */, int64_t expect_stride,
                           int64_t* report_dev /* rows * 4 */, void* hip_stream);
/* the samples one workgroup of the second launch covers: 8192 (0 for a null plan) */
int64_t wfk_segment_play_span(const wfk_segment_play_plan* plan);
/* launch 0: "segplay_check"; launch 1, 2, 3: the second launch of a play, of a verifying pass and of both,
 * "segplay_fill<1, true, false>", "segplay_fill<1, false, true>", "segplay_fill<1, true, true>" -- <width, out,
 * expect>; a static string ("" for another launch or a null plan) */
const char* wfk_segment_play_kernel_name(const wfk_segment_play_plan* plan, int launch);
int wfk_segment_play_plan_destroy(wfk_segment_play_plan* plan);

/* -- mixing across rows: a sparse matrix and an offset, per sample -------------------------------- */
/* rows_in real rows of n samples (kind: WFK_OUT_F64 or WFK_OUT_F32) become rows_out rows of the same kind through a
 * rows_out x rows_in matrix M and an offset per output row: flux crosstalk compensation (a band), IQ mixer correction
 * (2 x 2 blocks and a DC offset).  M comes as CSR: row_ptr[rows_out + 1] from 0 and non-decreasing, col[nnz] strictly
 * ascending inside a row, val[nnz] finite; offset: rows_out finite values, or NULL (all 0.0).  A TERM of output row o
 * is a pair (c, M[o, c]) with M[o, c] != 0 -- a zero, stored or not, is no term.  Per sample, in double (a float
 * sample is widened first) and without a fused multiply-add,
 *   acc = 0.0;   for the terms of o in ascending c:  acc = fl(acc + fl(x[c, i] * M[o, c]));
 *   y[o, i] = fl(acc + offset[o])          (a float result is rounded once, here)
 * -- what the NumPy loop `acc = acc + x[c] * m` computes, bit for bit.  An input row on which o has no term is not
 * read for o: its NaN and inf stay out of y[o] (a dense product would turn them into NaN).  A row without terms is
 * fl(0.0 + offset[o]).  rows_out < 1, rows_in < 1, n < 0, a row_ptr that is not non-decreasing from 0, a column out of
 * range ("row 3: column 9 is out of range"), columns that are not ascending, a coefficient or offset that is not
 * finite (the row is named), a kind other than F64 / F32, null pointers, more than 2^31 - 1 workgroups: WFK_EINVAL,
 * before any device work; no device: WFK_EHIP.
 * One kernel (mix_rows<T>): a workgroup owns a column span of a tile of WFK_MIX_TILE_ROWS consecutive output rows and
 * reads every input row the tile has a term on once.  wfk_mix_rows_reads(): the sum over tiles of the number of such
 * input rows -- the kernel reads reads * n and writes rows_out * n samples (block-diagonal blocks that divide the
 * tile: reads = rows_in; a band of half-width k: about (T + 2 k) / T * rows_in; dense: rows_in * tiles).
 * wfk_mix_rows_apply() allocates nothing and does not synchronise; strides are in elements, >= n, and may differ.
 * OUT OF PLACE only, and the input is never written: if [in, in + (rows_in - 1) * in_stride + n) meets
 * [out, out + (rows_out - 1) * out_stride + n), WFK_EINVAL; so are rows not aligned to their element.  n = 0: a
 * no-op that touches no pointer.  The plan owns its small tables and nothing else, so it may serve several streams. */
#define WFK_MIX_TILE_ROWS 8
typedef struct wfk_mix_rows_plan wfk_mix_rows_plan;
/* CSR: row_ptr[rows_out + 1], col[nnz] ascending inside a row, val[nnz]; offset may be NULL (all 0.0) */
int wfk_mix_rows_plan_create(int64_t n, int32_t rows_out, int32_t rows_in, int kind /* WFK_OUT_F64|F32 */,
                             const int64_t* row_ptr, const int32_t* col, const double* val,
                             const double* offset, wfk_mix_rows_plan** out);
int wfk_mix_rows_apply(wfk_mix_rows_plan* plan, const void* in_dev, int64_t in_stride,
                       void* out_dev, int64_t out_stride, void* hip_stream);
/* sum over tiles of the size of the input union; 0 for NULL */
int64_t wfk_mix_rows_reads(const wfk_mix_rows_plan* plan);
/* "mix_rows<double>" / "mix_rows<float>"; "" for NULL; a static string */
const char* wfk_mix_rows_kernel_name(const wfk_mix_rows_plan* plan);
int wfk_mix_rows_plan_destroy(wfk_mix_rows_plan* plan);       /* NULL is fine */

/* -- mixing across rows straight to DAC codes: wfk_mix_rows and wfk_dac_rows in one kernel --------- */
/* codes = wfk_dac_rows(wfk_mix_rows(in)) bit for bit -- codes and counts -- without the float rows between the two:
 * the matrix (CSR), mix_offset (rows_out values or NULL) and kind are those of wfk_mix_rows_plan_create; gain,
 * dac_offset (rows_out values each), bits, shift and interleave those of wfk_dac_rows_plan_create for batch =
 * rows_out.  Per sample, in double, without a fused multiply-add,
 *   acc = 0.0;   for the terms of o in ascending c:  acc = fl(acc + fl(x[c, i] * M[o, c]));   y = fl(acc + mix_offset[o])
 *   y = (double)(float)y     (kind F32 only: the two stages round the mixed row to float once)
 *   v = fl(fl(y * gain[o]) + dac_offset[o]),   q = rint(v),   c = 0 if v is NaN, lo if q < lo, hi if q > hi, else q
 *   out[g, i k + j] = ((int)c << shift as int16) of mix row o = g k + j   (k = interleave)
 * Every refusal of the two creators applies with its text, the mix's first, before any device work; no device:
 * WFK_EHIP.  One kernel, "mix_dac_rows<T,K,COUNT>": a workgroup owns a column span of a tile of
 * WFK_MIX_DAC_TILE_ROWS consecutive mix output rows (tile / k code rows) and reads every input row the tile has a term
 * on once; wfk_mix_dac_reads() is the sum over tiles of the number of such rows, so the kernel reads reads * n samples
 * and writes rows_out * n codes.  wfk_mix_dac_span(): the codes of one row a workgroup covers (4096 k).
 * wfk_mix_dac_apply() enqueues at most the zeroing of the counts and that kernel on `hip_stream`, and that is all it
 * does to the device (as wfk_chain_dac_launch: it may be called while the stream is being captured).  in_stride is in samples, >= n; out_stride in codes, >= k n where there is more than one code row;
 * counts_dev: NULL (the kernel then does no counting), or rows_out * 3 int64 [below, above, nan] per mix output row,
 * OVERWRITTEN by every apply.  OUT OF PLACE only, and the input is never written: out that meets in, or counts that
 * meet either, rows not aligned to their element, a stride below the row: WFK_EINVAL.  Nothing outside [0, n) of an
 * input row or [0, k n) of a code row is read or written.  n = 0: the kernel is not launched; the counts are still
 * zeroed.  The plan owns its small tables and nothing else, so it may serve several streams. */
#define WFK_MIX_DAC_TILE_ROWS 4
typedef struct wfk_mix_dac_plan wfk_mix_dac_plan;
int wfk_mix_dac_plan_create(int64_t n, int32_t rows_out, int32_t rows_in, int kind /* WFK_OUT_F64|F32 */,
                            const int64_t* row_ptr, const int32_t* col, const double* val,
                            const double* mix_offset /* or NULL */, const double* gain, const double* dac_offset,
                            int bits, int shift, int interleave, wfk_mix_dac_plan** out);
int wfk_mix_dac_apply(wfk_mix_dac_plan* plan, const void* in_dev, int64_t in_stride,
                      int16_t* out_dev, int64_t out_stride /* in codes, >= interleave * n */,
                      int64_t* counts_dev /* rows_out * 3, or NULL */, void* hip_stream);
/* sum over tiles of the size of the input union; 0 for NULL */
int64_t wfk_mix_dac_reads(const wfk_mix_dac_plan* plan);
/* the codes of one row a workgroup covers; 0 for NULL */
int64_t wfk_mix_dac_span(const wfk_mix_dac_plan* plan);
/* "mix_dac_rows<double,2,true>": T in {double, float}, K = interleave, COUNT = with_counts; "" for NULL; static */
const char* wfk_mix_dac_kernel_name(const wfk_mix_dac_plan* plan, int with_counts);
int wfk_mix_dac_plan_destroy(wfk_mix_dac_plan* plan);         /* NULL is fine */

/* -- per-row IIR straight to DAC codes: wfk_iir_rows and wfk_dac_rows in one kernel --------------- */
/* codes = wfk_dac_rows(wfk_iir_rows(in)) bit for bit -- codes, counts and zf -- without the float rows between the
 * two: a flux line without a crosstalk matrix, whose last float stage is its own exp-decay correction.  The sections,
 * n, batch and kind are those of wfk_iir_rows_plan_create (one cascade per row, equal-order sections, state dimension
 * <= 4); gain, offset (batch values each), bits and shift those of wfk_dac_rows_plan_create with interleave 1.  Per
 * sample
 *   y = the result of wfk_iir_rows_apply (kind F32: rounded to float once, as the two stages), widened to double
 *   v = fl(fl(y * gain[r]) + offset[r]),   q = rint(v),   c = 0 if v is NaN, lo if q < lo, hi if q > hi, else q
 *   out[r, i] = (int)c << shift as int16
 * Every refusal of the two creators applies with its text, the converter's first, before any device work; no device:
 * WFK_EHIP.  One kernel, "iir_rows_dac<T,NSEC,ORD>" (T: f64 / f32): a workgroup owns a row, walks it in tiles of 4096
 * samples through LDS as iir_rows_tile does and stores the tile as codes: in_elem + 2 bytes per sample.
 * wfk_iir_rows_dac_apply() enqueues that kernel on `hip_stream`, and that is all it does to the device (as
 * wfk_chain_dac_launch: it may be called while the stream is being captured).  in_stride is in samples, >= n; out_stride in
 * codes, >= n where there is more than one row; zi_dev / zf_dev / initial_dev as wfk_iir_rows_apply takes them;
 * counts_dev: NULL (the kernel then does no counting), or batch * 3 int64 [below, above, nan] per row, OVERWRITTEN by
 * every apply (the row's workgroup stores its totals: no zeroing in front).  OUT OF PLACE only, and the input is never
 * written: out that meets in, or counts that meet either, rows not aligned to their element, a stride below the row:
 * WFK_EINVAL.  Nothing outside [0, n) of a row is read or written; code rows may start at any 2-byte boundary
 * (16-byte stores where a row's slots are aligned, code by code elsewhere).  _apply_shared_in: every row reads the
 * SAME n samples at in_dev.  n = 0: the kernel is not launched; the counts are zeroed.  The plan owns its tables and
 * nothing else, so it may serve several streams. */
typedef struct wfk_iir_rows_dac_plan wfk_iir_rows_dac_plan;
int wfk_iir_rows_dac_plan_create(int32_t n_sections, const int32_t* orders, const double* b_rows,
                                 const double* a_rows, int64_t n, int32_t batch,
                                 int kind /* WFK_OUT_F64|F32 */, const double* gain, const double* offset,
                                 int bits, int shift, wfk_iir_rows_dac_plan** out);
int wfk_iir_rows_dac_apply(wfk_iir_rows_dac_plan* plan, const void* in_dev, int64_t in_stride,
                           int16_t* out_dev, int64_t out_stride /* in codes */,
                           int64_t* counts_dev /* batch * 3, or NULL */, const double* zi_dev, double* zf_dev,
                           const double* initial_dev, void* hip_stream);
int wfk_iir_rows_dac_apply_shared_in(wfk_iir_rows_dac_plan* plan, const void* in_dev, int16_t* out_dev,
                                     int64_t out_stride, int64_t* counts_dev, const double* zi_dev,
                                     double* zf_dev, const double* initial_dev, void* hip_stream);
int wfk_iir_rows_dac_state_dim(const wfk_iir_rows_dac_plan* plan);
/* "iir_rows_dac<f64,1,3>"; "" for NULL; owned by the plan */
const char* wfk_iir_rows_dac_kernel_name(const wfk_iir_rows_dac_plan* plan);
int wfk_iir_rows_dac_plan_destroy(wfk_iir_rows_dac_plan* plan);   /* NULL is fine */

/* -- sampler -> per-row IIR -> DAC codes: a whole flux line in one kernel ------------------------- */
/* wfk_chain_iir_rows_launch (WFK_OUT_F64) followed by wfk_dac_rows_apply, bit for bit -- codes, counts and zf. The
 * program, grid and sections are those of wfk_chain_iir_rows_plan_create; gain, offset (one per channel), bits and shift
 * those of wfk_dac_rows_plan_create with interleave 1; every refusal of the two with its text, the converter's first.
 * Where the chain plan fuses (wfk_chain_iir_rows_is_fused), the same fill runs in front of the codes store:
 * "iir_rows_sampled_dac<f64,NSEC,ORD>" on fine grids, "iir_rows_short_dac<f64,NSEC,ORD>" at AWG rates, 2 B per sample of
 * HBM traffic.  Otherwise (_unfused_reason) the sampler writes float64 rows into scratch_dev (n_channels rows,
 * scratch_stride >= n doubles apart, lent by the caller for the launch; it may meet neither the codes nor the counts)
 * and "iir_rows_dac<f64,NSEC,ORD>" reads them; a fused plan does not touch scratch_dev (NULL is fine).  zi_dev / zf_dev /
 * initial_dev as wfk_iir_rows_apply takes them; counts_dev as wfk_iir_rows_dac_apply.  A launch enqueues its one or two
 * kernels on `hip_stream`, and that is all it does to the device (it may be called while the stream is being captured).  n = 0: nothing is launched; the counts are zeroed. */
typedef struct wfk_chain_iir_rows_dac_plan wfk_chain_iir_rows_dac_plan;
int wfk_chain_iir_rows_dac_plan_create(const wfk_program* prog, const wfk_grid* grid, int32_t n_sections,
                                       const int32_t* orders, const double* b_rows, const double* a_rows,
                                       const double* gain, const double* offset, int bits, int shift,
                                       wfk_chain_iir_rows_dac_plan** out);
int wfk_chain_iir_rows_dac_launch(wfk_chain_iir_rows_dac_plan* plan, int16_t* out_dev, int64_t out_stride,
                                  int64_t* counts_dev /* n_channels * 3, or NULL */, void* scratch_dev,
                                  int64_t scratch_stride, const double* zi_dev, double* zf_dev,
                                  const double* initial_dev, void* hip_stream);
int wfk_chain_iir_rows_dac_is_fused(const wfk_chain_iir_rows_dac_plan* plan);
const char* wfk_chain_iir_rows_dac_unfused_reason(const wfk_chain_iir_rows_dac_plan* plan);   /* "" when fused */
const char* wfk_chain_iir_rows_dac_kernel_name(const wfk_chain_iir_rows_dac_plan* plan);
int64_t wfk_chain_iir_rows_dac_table_bytes(const wfk_chain_iir_rows_dac_plan* plan);
int wfk_chain_iir_rows_dac_state_dim(const wfk_chain_iir_rows_dac_plan* plan);
int wfk_chain_iir_rows_dac_plan_destroy(wfk_chain_iir_rows_dac_plan* plan);   /* NULL is fine */

/* -- per-row calibration curve: piecewise-linear lookup over sample VALUES ------------------------ */
/* `batch` real rows of n samples (kind: WFK_OUT_F64 or WFK_OUT_F32) go through a curve of their own: a flux pulse
 * programmed in its physical unit to volts through a measured monotone curve, an amplifier's compression table, a
 * DAC's INL table.  The curves come CSR-like: knot_ptr[batch + 1] from 0 and non-decreasing; row r has the
 * K = knot_ptr[r + 1] - knot_ptr[r] knots xp[knot_ptr[r] ..) -- finite, strictly increasing,
 * 2 <= K <= WFK_CURVE_MAX_KNOTS -- and the values fp[knot_ptr[r] ..), finite; rows may differ in K.  left / right:
 * batch doubles each, ANY double (NaN too), what a sample below xp[0] / above xp[K - 1] becomes; NULL: fp[0] / fp[K - 1]
 * of the row.  The host computes slope[j] = fl(fl(fp[j + 1] - fp[j]) / fl(xp[j + 1] - xp[j])) once, at creation.  Per
 * sample, in double (a float sample is widened first, the result rounded once) and without a fused multiply-add,
 *   x is NaN        -> y = x                                      (counted as nan)
 *   x < xp[0]       -> y = left                                   (below; -inf too)
 *   x > xp[K - 1]   -> y = right                                  (above; +inf too)
 *   j = the largest index with xp[j] <= x;   y = fp[j] if x == xp[j] (j = K - 1 is this case),
 *   y = fl(fl(slope[j] * fl(x - xp[j])) + fp[j]) otherwise
 * -- np.interp(x, xp, fp, left, right), bit for bit.  Departures from np.interp, on purpose: K = 1, knots that are
 * not finite or not strictly increasing and values that are not finite are refused.  n < 0, batch < 1, a knot_ptr
 * that is not non-decreasing from 0, a row with fewer than 2 or more than WFK_CURVE_MAX_KNOTS knots, such knots or
 * values (the row is named: "row 3: knots are not strictly increasing at 17"), a kind other than F64 / F32, null
 * pointers, more than 2^31 - 1 workgroups: WFK_EINVAL, before any device work; no device: WFK_EHIP.
 * wfk_curve_rows_apply() enqueues at most one memset (of the counts) and one kernel on `hip_stream`, and that is all
 * it does to the device.  Strides are in elements, >= n.  IN PLACE (out_dev == in_dev and out_stride == in_stride) or
 * out of place with extents that do not meet: [in, in + (batch - 1) * in_stride + n) meeting the same range of out in
 * any other way, rows not aligned to their element, null buffers: WFK_EINVAL.  counts_dev: NULL, or batch * 3 int64 on
 * the device, [below, above, nan] per row; every apply OVERWRITES them (zeroed on the stream, then added to with
 * integer atomics: bitwise reproducible); without them the kernel does no counting; counts that meet either side or
 * do not start at a multiple of 8: WFK_EINVAL.  n = 0: a no-op that still zeroes the counts.
 * One kernel (curve_rows<T>, with counts curve_rows_counts<T>): a workgroup copies its row's knots and a bucket table
 * over them into LDS and walks wfk_curve_rows_spans() consecutive spans of 2048 (F64) / 4096 (F32) samples of the row.
 * The plan owns its tables and nothing else, so it may serve several streams. */
#define WFK_CURVE_MAX_KNOTS 1024
typedef struct wfk_curve_rows_plan wfk_curve_rows_plan;
int wfk_curve_rows_plan_create(int64_t n, int32_t batch, int kind /* WFK_OUT_F64|F32 */,
                               const int64_t* knot_ptr /* batch + 1, from 0 */, const double* xp, const double* fp,
                               const double* left /* batch, or NULL */, const double* right /* batch, or NULL */,
                               wfk_curve_rows_plan** out);
int wfk_curve_rows_apply(wfk_curve_rows_plan* plan, const void* in_dev, int64_t in_stride, void* out_dev,
                         int64_t out_stride, int64_t* counts_dev /* batch * 3, or NULL */, void* hip_stream);
/* the spans one workgroup walks, chosen at creation from the size of the tables and of the grid; 0 for NULL */
int wfk_curve_rows_spans(const wfk_curve_rows_plan* plan);
/* "curve_rows<double>" / "curve_rows<float>", or with counts "curve_rows_counts<double>" /
 * "curve_rows_counts<float>"; "" for NULL; a static string */
const char* wfk_curve_rows_kernel_name(const wfk_curve_rows_plan* plan, int counts);
int wfk_curve_rows_plan_destroy(wfk_curve_rows_plan* plan);   /* NULL is fine */

/* -- per-row curve, IIR and DAC codes: a flux line's back end in one kernel ------------------------ */
/* codes = wfk_iir_rows_dac(wfk_curve_rows(in)) bit for bit -- codes, both reports and zf -- without the float rows
 * between them: the waveform in its physical unit through the line's measured curve to volts, the line's exp-decay
 * correction, the converter.  The curves (knot_ptr, xp, fp, left, right) are those of wfk_curve_rows_plan_create; the
 * sections, n, batch and kind those of wfk_iir_rows_plan_create; gain, offset, bits and shift those of
 * wfk_dac_rows_plan_create with interleave 1.  Per sample u = the result of wfk_curve_rows_apply (kind F32: rounded to
 * float once), then y and the code as wfk_iir_rows_dac_apply forms them from u; initial_dev holds levels of u.  Every
 * refusal of the three creators applies with its text -- the curve's first, then the converter's, then the cascades'
 * -- before any device work; no device: WFK_EHIP.  One kernel, "iir_rows_curve_dac<T,NSEC,ORD>": iir_rows_dac with the
 * row's knots and a bucket table copied into dynamic LDS once per row (static + dynamic <= 64 KiB: the bucket table
 * is the largest power of two, at most wfk_curve_rows' choice, that fits next to the tile -- down to none, plain
 * bisection; the count never changes a result) and every sample looked up on its way into the tile: in_elem + 2 bytes
 * per sample.  wfk_curve_iir_dac_apply() enqueues that kernel on `hip_stream`, and that is all it does to the device
 * (as wfk_iir_rows_dac_apply: it may be called while the stream is being captured).  Strides, zi_dev / zf_dev / initial_dev and counts_dev (the converter's [below, above, nan] per row) as
 * wfk_iir_rows_dac_apply takes them; beyond_dev: NULL, or batch * 3 int64, the CURVE's [below, above, nan] per row --
 * the samples of [0, n) outside the knots or NaN -- OVERWRITTEN by every apply like counts_dev (stored by the row's
 * workgroup: no zeroing in front).  OUT OF PLACE only: out that meets in, a report that meets either side or the other
 * report or does not start at a multiple of 8, rows not aligned to their element, a stride below the row: WFK_EINVAL.
 * _apply_shared_in: every row reads the SAME n samples at in_dev, each through its own curve and cascade.  n = 0: the
 * kernel is not launched; both reports are zeroed.  The plan owns its tables and nothing else. */
typedef struct wfk_curve_iir_dac_plan wfk_curve_iir_dac_plan;
int wfk_curve_iir_dac_plan_create(int32_t n_sections, const int32_t* orders, const double* b_rows,
                                  const double* a_rows, int64_t n, int32_t batch, int kind /* WFK_OUT_F64|F32 */,
                                  const int64_t* knot_ptr /* batch + 1, from 0 */, const double* xp, const double* fp,
                                  const double* left /* batch, or NULL */, const double* right /* batch, or NULL */,
                                  const double* gain, const double* offset, int bits, int shift,
                                  wfk_curve_iir_dac_plan** out);
int wfk_curve_iir_dac_apply(wfk_curve_iir_dac_plan* plan, const void* in_dev, int64_t in_stride, int16_t* out_dev,
                            int64_t out_stride /* in codes */, int64_t* counts_dev /* batch * 3, or NULL */,
                            int64_t* beyond_dev /* batch * 3, or NULL */, const double* zi_dev, double* zf_dev,
                            const double* initial_dev, void* hip_stream);
int wfk_curve_iir_dac_apply_shared_in(wfk_curve_iir_dac_plan* plan, const void* in_dev, int16_t* out_dev,
                                      int64_t out_stride, int64_t* counts_dev, int64_t* beyond_dev,
                                      const double* zi_dev, double* zf_dev, const double* initial_dev,
                                      void* hip_stream);
int wfk_curve_iir_dac_state_dim(const wfk_curve_iir_dac_plan* plan);
/* "iir_rows_curve_dac<f64,1,3>"; "" for NULL; owned by the plan */
const char* wfk_curve_iir_dac_kernel_name(const wfk_curve_iir_dac_plan* plan);
int wfk_curve_iir_dac_plan_destroy(wfk_curve_iir_dac_plan* plan);   /* NULL is fine */

/* -- sampler -> per-row curve -> per-row IIR -> DAC codes: a flux line in its physical unit --------- */
/* wfk_plan_launch (WFK_OUT_F64), wfk_curve_rows_apply in place and wfk_iir_rows_dac_apply, bit for bit -- codes, both
 * reports and zf.  The program, grid and sections are those of wfk_chain_iir_rows_dac_plan_create, the curves those of
 * wfk_curve_rows_plan_create (one per channel), gain, offset, bits and shift the converter's; every refusal with its
 * text, the curve's first, then the converter's, then the chain's, before any device work.  Fused (_is_fused) exactly
 * where wfk_chain_iir_rows_dac is, with its reasons -- and one more: a curve of more than 567 knots does not fit next to
 * the fine-grid fill's LDS.  Fused, every sample the fill produces goes through its row's curve before it enters the
 * filter: "iir_rows_sampled_curve_dac<f64,NSEC,ORD>" on fine grids, "iir_rows_short_curve_dac<f64,NSEC,ORD>" at AWG
 * rates, 2 B per sample of HBM traffic, static + dynamic LDS <= 64 KiB.  Otherwise (_unfused_reason) the sampler writes
 * float64 rows into scratch_dev (as wfk_chain_iir_rows_dac_launch takes it; it may meet neither the codes nor a report)
 * and "iir_rows_curve_dac<f64,NSEC,ORD>" reads them.  counts_dev / beyond_dev as wfk_curve_iir_dac_apply takes them.  A
 * launch enqueues its one or two kernels on `hip_stream`, and that is all it does to the device (it may be called
 * while the stream is being captured).  n = 0: nothing is launched; both reports are zeroed. */
typedef struct wfk_chain_curve_iir_dac_plan wfk_chain_curve_iir_dac_plan;
int wfk_chain_curve_iir_dac_plan_create(const wfk_program* prog, const wfk_grid* grid, int32_t n_sections,
                                        const int32_t* orders, const double* b_rows, const double* a_rows,
                                        const int64_t* knot_ptr /* n_channels + 1, from 0 */, const double* xp,
                                        const double* fp, const double* left /* n_channels, or NULL */,
                                        const double* right /* n_channels, or NULL */, const double* gain,
                                        const double* offset, int bits, int shift,
                                        wfk_chain_curve_iir_dac_plan** out);
int wfk_chain_curve_iir_dac_launch(wfk_chain_curve_iir_dac_plan* plan, int16_t* out_dev, int64_t out_stride,
                                   int64_t* counts_dev /* n_channels * 3, or NULL */,
                                   int64_t* beyond_dev /* n_channels * 3, or NULL */, void* scratch_dev,
                                   int64_t scratch_stride, const double* zi_dev, double* zf_dev,
                                   const double* initial_dev, void* hip_stream);
int wfk_chain_curve_iir_dac_is_fused(const wfk_chain_curve_iir_dac_plan* plan);
const char* wfk_chain_curve_iir_dac_unfused_reason(const wfk_chain_curve_iir_dac_plan* plan);   /* "" when fused */
const char* wfk_chain_curve_iir_dac_kernel_name(const wfk_chain_curve_iir_dac_plan* plan);
int64_t wfk_chain_curve_iir_dac_table_bytes(const wfk_chain_curve_iir_dac_plan* plan);
int wfk_chain_curve_iir_dac_state_dim(const wfk_chain_curve_iir_dac_plan* plan);
int wfk_chain_curve_iir_dac_plan_destroy(wfk_chain_curve_iir_dac_plan* plan);   /* NULL is fine */

/* -- per-row kernel extraction: the reference's extractKernel for every row ---------------------- */
/* ker[r] = extractKernel(sig_in[r], sig_out[r], sample_rate, bw, skip) (waveforms/distortion.py:42-48) for `batch`
 * rows of n doubles: the kernel that maps sig_out back onto sig_in, the rows of an FIR plan's kernel matrix.  Per row
 *   R[k] = rfft(sig_in)[k] / rfft(sig_out)[k] / n, k = 0 .. n/2;   c = irfft(R, n);   s[i] = c[(i + n/2) mod n];
 *   t[i] = sum_m taps[m] s[i + (n_taps - 1)/2 - m], s = 0 outside [0, n)  (np.convolve(s, taps, 'same'); t = s for
 *   n_taps = 0);   ker[j] = t[j + skip], 0 <= j < K = max(n - 2 skip, 0).
 * The caller computes the taps with the reference's expression, M = int(2 * sample_rate / bw) points of
 * exp(-0.5 * linspace(-3, 3, M)**2) divided by their sum, when bw is given and bw < sample_rate / 2; n_taps = 0
 * otherwise.  in_rows = 1: ONE sig_in row shared by all rows (it is transformed once per apply); in_rows = batch:
 * one per row.  Two departures from the reference, on purpose: n_taps > n is refused (np.convolve 'same' returns
 * n_taps samples there; rows keep their length here) and so is skip < 0 (the reference's slice then means
 * something else).  n < 1, batch < 1, in_rows not 1 or batch, skip < 0, n_taps < 0 or > n, a tap that is not finite,
 * null pointers: WFK_EINVAL; no device: WFK_EHIP.  A zero bin in the transform of a sig_out row makes that row's
 * result non-finite, as in the reference; other rows are not touched by it.
 * The plan owns the rocFFT plans, the staging and spectrum buffers and the taps.  wfk_extract_rows_apply() allocates
 * nothing and does not synchronise; strides are in elements, >= n for the signals and >= K for the result; one plan
 * serves one stream at a time.  Both inputs are staged first, so they may overlap each other in any way; the result
 * [ker, ker + (batch - 1) * ker_stride + K) may overlap neither input: WFK_EINVAL.  K = 0: a no-op.
 * Two kernels around rocFFT: extract_ratio (one pass over the two R2C outputs) and extract_smooth (rotation,
 * smoothing and crop in one pass from the C2R output to ker; without taps it moves values bit for bit; with taps
 * every output adds its products in ascending m, so a row's result does not depend on the tile or the batch). */
typedef struct wfk_extract_rows_plan wfk_extract_rows_plan;
int wfk_extract_rows_plan_create(int64_t n, int32_t batch, int32_t in_rows /* 1 or batch */, const double* taps_host,
                                 int32_t n_taps /* 0: no smoothing */, int64_t skip, wfk_extract_rows_plan** out);
int wfk_extract_rows_apply(wfk_extract_rows_plan* plan, const double* sig_in_dev, int64_t in_stride,
                           const double* sig_out_dev, int64_t out_sig_stride, double* ker_dev, int64_t ker_stride,
                           void* hip_stream);
/* "extract_ratio + extract_smooth"; a static string */
const char* wfk_extract_rows_kernel_name(const wfk_extract_rows_plan* plan);
int wfk_extract_rows_plan_destroy(wfk_extract_rows_plan* plan);

/* -- readout demodulation (reference utils.py:35-84: traces @ getFTMatrix(...)) ---------------- */
/* out[s, j] = sum_k x[s, k] * e[k, j] for real traces x (n_shots rows of >= n_points samples, row stride
 * trace_stride elements) and a complex matrix e (n_points x n_freq, complex128 interleaved, point-major: the
 * memory of NumPy's (N, nf) complex128 array).  fp64 arithmetic throughout; int16 codes are exact in fp64.
 * The plan uploads e once (zero-padded column blocks); out is complex128, row stride out_stride complex
 * elements, 16-byte aligned.  Small n_shots split n_points across workgroups into a workspace the plan owns,
 * reduced in a fixed order (bitwise reproducible for a given shape).  wfk_demod_apply() allocates nothing and
 * does not synchronise; use one plan per concurrent stream.                                               */
enum { WFK_IN_F64 = 0, WFK_IN_F32 = 1, WFK_IN_I16 = 4 };
typedef struct wfk_demod_plan wfk_demod_plan;
int wfk_demod_plan_create(const double* e_host, int64_t n_points, int32_t n_freq, int in_kind,
                          wfk_demod_plan** out);
int wfk_demod_apply(wfk_demod_plan* p, const void* traces_dev, int64_t n_shots, int64_t trace_stride,
                    void* out_dev, int64_t out_stride, void* hip_stream);
/* "demod_tile<T,NB>", with " + demod_reduce" when a launch of n_shots splits n_points; the string lives
 * until the next call on this plan                                                                      */
const char* wfk_demod_kernel_name(const wfk_demod_plan* p, int64_t n_shots);
int wfk_demod_plan_destroy(wfk_demod_plan* p);

/* -- readout demodulation per time bin: the IQ trajectory of every shot --------------------------- */
/* out[s, w, j] = sum over the samples k of bin w of x[s, k] * e[k, j], bin w = [start + w * bin, start + (w + 1) * bin),
 * w = 0 .. bins - 1, with start >= 0, bin >= 1, bins >= 1 and start + bins * bin <= n_points: traces and e as
 * wfk_demod_plan_create takes them (e keeps the global time axis, so the phases run on from bin to bin), fp64
 * arithmetic throughout.  out is n_shots x bins x n_freq complex128, dense within a shot, shots out_stride >= bins *
 * n_freq complex elements apart, 16-byte aligned: out[:, w] is a points matrix as wfk_states_apply takes it (row stride
 * out_stride).  Samples before `start` and behind the last bin are not read; a sample outside a bin is left out of
 * the sum, not multiplied by zero, so a NaN or Inf in sample k of shot s reaches out[s, bin of k, :] and nothing else.
 * The rows [start, start + bins * bin) of e must be finite (a zero-filled position of the kernel multiplies them);
 * the first entry that is not is named in the refusal.  The plan uploads these rows once (zero-padded column blocks).
 * A bin is summed by one wave in a fixed order: no float atomics, no workspace, no second kernel, and two applies of one
 * call agree to the bit.  wfk_bdemod_apply() enqueues one kernel (bdemod_tile) on `hip_stream`, and that is all it does
 * to the device (as wfk_avg_apply: it may be called while the stream is being captured); n_shots = 0 enqueues nothing.
 * The plan owns no scratch: it may serve several streams at once.
 * WFK_EINVAL, before any device work: n_points < 1, n_freq < 1, bin < 1, bins < 1, start < 0, start + bins * bin >
 * n_points (tested without a product), bins * n_freq above 2^31 - 1, a bad in_kind, a used entry of e that is not
 * finite; n_shots < 0, trace_stride < n_points with more than one shot, out_stride < bins * n_freq, a null or
 * misaligned side, out overlapping the traces.  No device: WFK_EHIP, after these. */
typedef struct wfk_bdemod_plan wfk_bdemod_plan;
int wfk_bdemod_plan_create(const double* e_host, int64_t n_points, int32_t n_freq, int in_kind,
                           int64_t start, int64_t bin, int64_t bins, wfk_bdemod_plan** out);
int wfk_bdemod_apply(wfk_bdemod_plan* p, const void* traces_dev, int64_t n_shots, int64_t trace_stride,
                     void* out_dev, int64_t out_stride /* complex elements per shot */, void* hip_stream);
/* workgroups along the bin axis for a block of n_shots: a function of the shape alone, no plan, no device.  A workgroup
 * owns 64 shots, one block of NB = 4 / 8 / 16 / 32 tones (the least that holds n_freq, 32 above) and one group of
 * consecutive bins.  With blocks = ceil(n_shots / 64) * ceil(n_freq / NB): g = max(1, 1024 / blocks) groups bring the
 * launch to about 1024 workgroups, at most max(1, bins / 4) of them so that a group keeps four bins (one per wave) where
 * bins allows, both divisions rounding down; a group then holds per = ceil(bins / g) bins and the answer is
 * ceil(bins / per).  0 for n_shots < 1, n_freq < 1 or bins < 1 */
int64_t wfk_bdemod_bin_groups(int64_t n_shots, int32_t n_freq, int64_t bins);
/* "bdemod_tile<T,NB> groups=G", G = wfk_bdemod_bin_groups(n_shots, ...); the string lives until the next call on this
 * plan; "" for NULL */
const char* wfk_bdemod_kernel_name(const wfk_bdemod_plan* p, int64_t n_shots);
int wfk_bdemod_plan_destroy(wfk_bdemod_plan* p);   /* NULL is fine */

/* -- per-step shot sums of readout traces: the reduction over shots ------------------------------ */
/* A block of n_shots traces (rows of >= n_points samples of in_kind, row stride trace_stride elements) taken while a
 * sequence cycled through `steps` steps, `first` shots of the run before it: shot s of the block belongs to step
 * (first + s) mod steps; a block may start and end anywhere in a cycle, n_shots < steps and n_shots = 0 are fine.
 * Per step g and column c, over the block's shots of that step:  sum[g, c] = SUM x[s, c],  sumsq[g, c] = SUM x[s, c]^2
 * -- int64 for WFK_IN_I16 codes (exact), fp64 for WFK_IN_F32 / WFK_IN_F64 (a float32 sample is widened first, so its
 * square is exact).  sum and sumsq (NULL: none) are the caller's, `steps` rows of n_points 8-byte elements, row
 * strides in elements.  accumulate = 0 OVERWRITES every element of both (a step without a shot in the block gets 0);
 * accumulate != 0 ADDS the block's sums to what is there -- the block's sum is formed first, then added with one add
 * per element -- and leaves a step without a shot in the block bit for bit as it was: the way to carry sums across
 * the blocks a digitiser delivers.  No atomics: the order of the float additions is a fixed function of (n_shots,
 * steps, n_points, first mod steps, in_kind), so two applies of one call agree to the bit; a NaN or Inf in a sample
 * reaches its own (step, column) only.
 * wfk_avg_apply() enqueues one kernel (avg_tile) or two (avg_tile into the plan's workspace, then avg_reduce: a block
 * whose column tiles and steps alone do not fill the chip splits the shots of a step over wfk_avg_splits() workgroups)
 * on `hip_stream`, and that is all it does to the device (as wfk_curve_rows_apply: it may be called while the stream
 * is being captured, and every replay reads an accumulate base anew).  The plan owns that workspace, taken at
 * creation (8 to 34 MB by in_kind): one plan per concurrent stream.
 * WFK_EINVAL: n_points < 1, steps < 1, a stride < n_points, n_shots < 0, first < 0, null or misaligned rows, sum or
 * sumsq overlapping the traces or each other.  No device: WFK_EHIP. */
typedef struct wfk_avg_plan wfk_avg_plan;
int wfk_avg_plan_create(int64_t n_points, int64_t steps, int in_kind /* WFK_IN_F64|F32|I16 */, wfk_avg_plan** out);
int wfk_avg_apply(wfk_avg_plan* plan, const void* traces_dev, int64_t n_shots, int64_t trace_stride, int64_t first,
                  void* sum_dev, int64_t sum_stride, void* sumsq_dev /* NULL: none */, int64_t sumsq_stride,
                  int accumulate, void* hip_stream);
/* the workgroups that share the shots of one step for a block of n_shots (1: avg_tile writes the outputs itself): with
 * T = ceil(n_points / (256 * 16 / sizeof(sample))) column tiles, min(1024 / T / steps, ceil(n_shots / steps) / 32),
 * at least 1; the environment's WFK_AVG_SPLITS = k, read at creation, asks for k in place of the second term (an
 * experiment's switch).  0 for NULL */
int64_t wfk_avg_splits(const wfk_avg_plan* plan, int64_t n_shots, int64_t first);
/* "avg_tile<short|float|double>" or "avg_tile<...,sumsq>", with " + avg_reduce" when a block of n_shots splits; the
 * string lives until the next call on this plan; "" for NULL */
const char* wfk_avg_kernel_name(const wfk_avg_plan* plan, int64_t n_shots, int with_sumsq);
int wfk_avg_plan_destroy(wfk_avg_plan* plan);   /* NULL is fine */

/* -- IQ points to qubit states and per-step counts: the link behind the demodulator -------------- */
/* points: n_shots rows of n_tones complex128 IQ points (the demodulator's output as it is; row stride points_stride
 * complex elements, 16-byte aligned); centres: n_tones x n_states complex128 on the host, 2 <= n_states <= 8,
 * 1 <= n_tones <= 1024; a tone with fewer states pads its row with NaN centres.  Per shot s, tone j, state k, in
 * double, every operation rounded on its own (two subtractions, two products, one addition, no fused multiply-add --
 * the bits of NumPy's dr * dr + di * di):
 *   dr = re(p) - re(c),  di = im(p) - im(c),  d2 = dr * dr + di * di
 * and walking k = 0 .. n_states - 1 from best = +inf, k wins when d2 < best (strict): ties go to the lowest k, a NaN
 * or infinite d2 (a NaN centre, a NaN or Inf point, a distance that overflows) never wins, a point no centre wins
 * gets label 255 ("invalid"), -0.0 behaves as 0.0.  With b = 1 for n_states = 2, 2 for <= 4, 3 for <= 8 bits per tone,
 * the outputs -- all the caller's, NULL for each one not wanted, at least one -- are
 *   labels  n_shots rows of n_tones uint8, row stride labels_stride
 *   words   n_shots int64: tone j in bits [j b, (j + 1) b); -1 when a tone of the shot is invalid; n_tones * b <= 62
 *   counts  steps x n_tones x (n_states + 1) int64, contiguous: counts[g, j, k] = the block's shots of step g whose
 *           tone j got state k, column n_states the invalid ones
 *   joint   steps x (2^(n_tones b) + 1) int64, contiguous: bin w = the shots of step g whose word is w, the last bin
 *           those with word -1; codes no state produces stay 0; n_tones * b <= 16
 * Shot s of the block belongs to step (first + s) mod steps, `first` shots of the run before it (any int64 >= 0): a
 * block may start and end anywhere in a cycle, n_shots < steps and n_shots = 0 are fine.  accumulate = 0 OVERWRITES
 * every element of counts and joint (a step without a shot gets 0; they are zeroed by a kernel on the stream, then
 * added to); accumulate != 0 ADDS the block's counts to what is there: the way to carry counts across the blocks a
 * digitiser delivers.  All sums are integers (64-bit atomic adds): the tables do not depend on the order of arrival;
 * labels and words are a pure function of the inputs.
 * wfk_states_apply() enqueues at most two zeroing kernels and one kernel (states_block) on `hip_stream`, and that is
 * all it does to the device (as wfk_curve_rows_apply: it may be called while the stream is being captured, and every
 * replay reads an accumulate base anew).  The plan owns its table of centres and nothing else, so it may serve several
 * streams.
 * WFK_EINVAL, before any device work: n_tones outside [1, 1024], n_states outside [2, 8], steps < 1, steps * n_tones *
 * (n_states + 1) above 2^31 - 1, a tone without a finite centre (the tone is named); n_shots < 0, first < 0, no output
 * at all, words with n_tones * b > 62, joint with n_tones * b > 16 or more than 2^31 - 1 entries, a stride below
 * n_tones, null or misaligned rows, an output that overlaps the points or another output.  No device: WFK_EHIP. */
#define WFK_STATES_MAX_TONES 1024
#define WFK_STATES_MAX_STATES 8
typedef struct wfk_states_plan wfk_states_plan;
int wfk_states_plan_create(const double* centres_host /* n_tones * n_states complex128, interleaved */,
                           int32_t n_tones, int32_t n_states, int64_t steps, wfk_states_plan** out);
int wfk_states_apply(wfk_states_plan* plan, const void* points_dev, int64_t n_shots, int64_t points_stride,
                     int64_t first, uint8_t* labels_dev /* or NULL */, int64_t labels_stride,
                     int64_t* words_dev /* or NULL */, int64_t* counts_dev /* or NULL */,
                     int64_t* joint_dev /* or NULL */, int accumulate, void* hip_stream);
/* "states_block<KT> tile=T counts:lds|global joint:lds|global|none": KT = n_states rounded up to 2, 4 or 8; T the
 * points of a workgroup's block for n_shots (4096, halved down to 1024 while the launch has fewer than 1024
 * workgroups); where each table is counted -- in a per-workgroup LDS histogram when it has at most 4096 entries, by
 * global atomic adds otherwise, a function of the plan's shape alone; the environment's WFK_STATES_COUNTERS = global,
 * read at creation, takes every table to global memory (= lds asks for the rule; an experiment's and the tests'
 * switch).  The string lives until the next call on this plan; "" for NULL */
const char* wfk_states_kernel_name(const wfk_states_plan* plan, int64_t n_shots);
int wfk_states_plan_destroy(wfk_states_plan* plan);   /* NULL is fine */

/* -- boxcar integral read off at probe times (reference distortion.py:349-366: the tail of phase_curve) ----- */
/* out[r, q] = np.interp(t_q, tlist, conv[r]) with conv[r, i] = gain * sum_{m < pp} y[r, i + c - m] (y zero outside
 * [0, n)) -- np.convolve(s, [ones(pp), zeros(sp)], 'same') for c = (pp + sp - 1) / 2 -- for every row of y
 * (n_rows rows of >= n doubles, row stride y_stride elements) and every one of the n_query probe times, without
 * forming conv: a probe needs it at its two bracketing grid points only.  The plan is built on the host from the
 * caller's own tlist[0..n) (ascending, no NaN) and t[0..n_query): per query the bracket index j, dx = t - tlist[j]
 * and w = tlist[j + 1] - tlist[j] by np.interp's rules (t outside the grid takes the first / last grid value, a NaN
 * t gives NaN, t in any order), uploaded once.  out[r, q] = f0 + (f1 - f0) / w * dx with f_i = gain * (the pp samples
 * ending at j + i + c).  fp64 throughout; out is (n_rows, n_query) doubles, row stride out_stride elements.
 * One kernel (boxprobe_wave): a wave per (row, query), lanes stride the pp + 1 samples both windows share, partial
 * sums added in a fixed order, no atomics: bitwise reproducible, equal rows give equal results wherever they sit.
 * wfk_boxprobe_apply() allocates nothing and does not synchronise; a plan holds no scratch and may serve several
 * streams.  wfk_boxprobe_brackets() is the host-only table builder the plan uses (no device needed).              */
typedef struct wfk_boxprobe_plan wfk_boxprobe_plan;
int wfk_boxprobe_brackets(const double* tlist, int64_t n, const double* t, int64_t n_query, int64_t* j_out,
                          double* dx_out, double* w_out);
int wfk_boxprobe_plan_create(const double* tlist_host, int64_t n, const double* t_host, int32_t n_query,
                             int64_t pp, int64_t c, double gain, wfk_boxprobe_plan** out);
int wfk_boxprobe_apply(wfk_boxprobe_plan* p, const double* y_dev, int64_t n_rows, int64_t y_stride,
                       double* out_dev, int64_t out_stride, void* hip_stream);
/* "boxprobe_wave" */
const char* wfk_boxprobe_kernel_name(const wfk_boxprobe_plan* p);
int wfk_boxprobe_plan_destroy(wfk_boxprobe_plan* p);

/* -- pinned host blocks for results ------------------------------------------------------- */
/* Page-locked host memory from a per-process cache (power-of-two blocks, parked on free).  A result
 * buffer taken from here costs no page faults, takes the D2H DMA directly and lets wfk_plan_run_host
 * overlap the copy of one part of a big single-channel result with the kernel of the next -- what the
 * drop-in calls Waveform.__call__ / Waveform.sample (waveforms/waveform.py:529-563, 173-207) need at
 * 1e7 points.  wfk_plan_run_host accepts any host pointer; only blocks from here get the pipeline.  */
int wfk_host_alloc(void** host_ptr, size_t bytes);
int wfk_host_free(void* host_ptr);

/* 1 if every one of the n 64-bit floats at `host` is finite, 0 if one is NaN or +-inf (a few host threads;
 * ~1 ms for 80 MB).  `Waveform.__call__(x, out=buf)` zeroes the caller's array with `out *= 0`
 * (waveforms/waveform.py:551), which KEEPS NaN / inf: the drop-in call asks this before it lets
 * wfk_plan_run_host overwrite `buf`, and follows the reference's two passes when the answer is 0.   */
int wfk_host_all_finite(const double* host, int64_t n);

/* -- device memory helpers for FFI callers without a HIP binding ---------- */
int wfk_malloc(void** dev_ptr, size_t bytes);
int wfk_free(void* dev_ptr);
int wfk_memcpy_h2d(void* dst_dev, const void* src_host, size_t bytes);
int wfk_memcpy_d2h(void* dst_host, const void* src_dev, size_t bytes);
int wfk_memset(void* dst_dev, int byte, size_t bytes);
int wfk_stream_sync(void* hip_stream);

#ifdef __cplusplus
}
#endif
#endif /* WFK_H */
