// wfk_short_body.inc -- the body of wfk_sample_short and wfk_sample_short_dac (wfk_short.hip, which says why it is a
// text and not a function): T, CPLX, ACC, R, FAM, DAC, COUNT, `a` (SArgs) and `dk` (DacKArgs) come from the kernel.
  using E = typename std::conditional<DAC, int16_t, typename std::conditional<CPLX, typename ShOut<T>::Cplx, T>::type>::type;
  // float launches of the plain pulse train (family 3 = family 0 in packed fp32 arithmetic, wfk_short_dev.h: short_op_pk)
  constexpr bool PK = FAM == 3;
  // what a family holds beside the carrier-envelope ops: F1 closing ops of flat tops / multi-tone pieces and linear chirps,
  // F2 table / mollifier envelopes, F4 exponential / hyperbolic chirp multipliers (libm log behind a call: a family of
  // its own, so that the table envelopes keep their register allocation)
  constexpr bool F1 = FAM == 1 || FAM == 2 || FAM == 4, F2 = FAM == 2 || FAM == 4, F4 = FAM == 4;
  // family 6 = family 0 + carriers with the grid-rounding correction (pulse trains milliseconds from t = 0: short_op_corr)
  constexpr bool F6 = FAM == 6;
  static_assert(!PK || (std::is_same<T, float>::value && !CPLX), "packed arithmetic: real float launches only");
  __shared__ __attribute__((aligned(16))) E s_out[kStage];
  const int lane = threadIdx.x;
  // XCD-aware chunk map (workgroup b runs on XCD b % 8): XCD x walks the x-th contiguous eighth
  const int64_t b = blockIdx.x;
  const int64_t per = (a.n_chunks + 7) >> 3;
  const int64_t lchunk = (b & 7) * per + (b >> 3);
  if (lchunk >= a.n_chunks) return;
  const int64_t chunk = a.chunk_base + lchunk;
  const int64_t u0 = chunk * a.units_per_chunk;
  const int64_t u1 = u0 + a.units_per_chunk < a.n_units ? u0 + a.units_per_chunk : a.n_units;
  const int64_t ulast = a.n_units - 1;

  auto slot_of = [&](const UnitDesc& d) -> uint32_t {     // lanes >= nslots read 0: no segment
    return buf_load<uint32_t>(make_rsrc(a.slots + d.slot0, (unsigned)d.nslots * 4u), lane * 4);
  };
  // (len, o, first sample's index, record) of this lane's segment
  struct Seg { int len, o, j; const double* rec; };
  auto decode = [&](uint32_t slot, const UnitDesc& d) -> Seg {
    Seg g;
    g.len = (slot >> 31) ? (int)((slot >> 26) & 15) + 1 : 0;
    g.o = (int)((slot >> 16) & 0x3ff);
    g.j = (int)(uint32_t)d.j0 + g.o;
    g.rec = a.recs + 2 * (d.rec0 + (int64_t)(slot & 0xffff));
    return g;
  };

  // The pipeline fills INSIDE the loop: iteration u0 - 1 works on an empty unit (no slots, zero samples:
  // the range check drops its stores).  With a separate prologue the compiler merges two histories at the
  // loop header and waits for the record as if only the prologue's single load followed it (vmcnt(1):
  // every store of the previous unit), instead of leaving the 16 stores and the slot load in flight.
  UnitDesc cur{};
  UnitDesc nxt = load_unit(a.units + u0);
  Seg seg{0, 0, 0, a.recs};
  OpRec first{};
  [[maybe_unused]] double dgain = 0.0, doffset = 0.0;     // DAC build: the row of `cur`

  for (int64_t ui = u0 - 1; ui < u1; ++ui) {
    // two units ahead: descriptor; one ahead: slot words (none past the end of the chunk)
    const UnitDesc nn = load_unit(a.units + (ui + 2 <= ulast ? ui + 2 : ulast));
    if (ui + 1 >= u1) { nxt.nslots = 0; nxt.ns = 0; }
    const uint32_t nslot = slot_of(nxt);
    [[maybe_unused]] double ngain = 0.0, noffset = 0.0;   // ... and of the next unit: in flight with its slot words
    if constexpr (DAC) {
      ngain = cload<double>(dk.rows, (int64_t)nxt.ch * 16);
      noffset = cload<double>(dk.rows, (int64_t)nxt.ch * 16 + 8);
    }
    E* const orow = uniptr(reinterpret_cast<E*>(a.out) + (int64_t)cur.ch * a.ch_stride + cur.j0);
    const int head = (int)(cur.j0 & 15);     // rows start on 16-sample boundaries (whole 128-B lines for fp64)
    const int ns = cur.ns;
    E fillv;
    [[maybe_unused]] unsigned fill_rails = 0, fill_nan = 0;   // DAC build: how the channel's constant counts
    [[maybe_unused]] int dhead = 0;                           // ... and the unit's first code's place in its group of 8
    [[maybe_unused]] unsigned cnt_rails = 0, cnt_nan = 0;     // ... this lane's run: below | above << 16, nan
    if constexpr (DAC) {
      fillv = dac_code(cur.offset, dgain, doffset, dk.lo, dk.hi, dk.shift, fill_rails, fill_nan);
      dhead = (int)((reinterpret_cast<uintptr_t>(orow) >> 1) & 7);
    } else
    if constexpr (CPLX) { fillv.x = (T)cur.offset; fillv.y = (T)0; } else { fillv = (T)cur.offset; }
    const int l0 = lane - head;                 // this lane's sample in row 0 (negative: before the unit)
    // Staging layout, chosen per unit by the host for the unit's own segment offsets: plain (sample i at
    // element i: conflict-free when the runs start an odd number of samples apart, e.g. 15), or padded by
    // one element per 16 (i + (i >> 4): runs of 16 then start 17 apart).  Either way row r, lane x sits at
    // rs * r + f(x), one per-lane base and a uniform row stride.
    const bool sw = (cur.gaps & 2) != 0;
    const int rs = sw ? 68 : 64;
    const int s0 = sw ? l0 + (l0 >> 4) : l0;    // (arithmetic shift: exact for the negative l0 of row 0 too)

    double acc[PK ? 1 : R], acci[CPLX ? R : 1];
    f32x2 accp[PK ? R / 2 : 1];
    SH_EACH(PK ? 1 : R, k) acc[k] = 0.0; SH_END
    SH_EACH(CPLX ? R : 1, k) acci[k] = 0.0; SH_END
    SH_EACH(PK ? R / 2 : 1, k) accp[k] = 0.0f; SH_END

    if (cur.nslots != 0) {
      const double kf = (double)(seg.j - op_ref(first));   // samples from the record's reference sample
      const double* op = seg.rec;
      OpRec rec = first;
      bool live = seg.len > 0;
      // The first op is evaluated in straight-line code, further ops (multi-tone pieces) in a loop:
      // a loop whose body reads registers loaded before it gets a vmcnt(0) in its preheader from the
      // compiler (SIInsertWaitcnts' preheader flush), which here would wait for the slot load just
      // issued and for every store of the previous unit.
      auto eval = [&](const OpRec& rc, const double* opp, bool lv) -> bool {   // -> another op follows
        // (the unused halves of the record stay "live" up to here: registers that die at the load are
        //  handed out again as temporaries while the load is still in flight, and writing them means
        //  waiting for it -- a vmcnt(3) right behind the prefetch)
        asm volatile("" : : "v"(rc.a.x));
        const int w = op_word(rc);
        const bool closing = ((w >> 4) & 3) == 3;       // closing multiplier (erf edge, table, mollifier)
        const bool mine = lv && !closing && (CPLX || !(w & 8));   // op of the imaginary part: a real launch keeps .real
        const bool chirp = F1 && (w & 512) != 0;  // quadratic phase (16-double record, polynomials of degree <= 1)
        const bool cubic = __any(mine && !chirp && (w & 3) > 1 && !(F6 && (w & 4096)));
        if constexpr (PK) {
          if (mine) {
            if (cubic) short_op_pk<R, true>(rc, opp, w, kf, a.step, accp);
            else short_op_pk<R, false>(rc, opp, w, kf, a.step, accp);
          }
          return lv && !(w & WFK_SH_LAST);
        } else {
        if constexpr (F1) {
          if (__any(mine && chirp)) {
            if (mine && chirp) short_chirp<R, CPLX>(rc, opp, w, kf, a.step, acc, acci);
          }
        }
        // bare carriers (degree 0, no envelope): the tones of a multi-tone piece, plateaus -- half the instructions per sample
        const bool bare = F1 && !chirp && (w & 0x33) == 0 && (w & 4) != 0;
        if constexpr (F1) {
          if (__any(mine && bare)) {
            if (mine && bare) short_op_bare<R, CPLX>(rc, w, kf, acc, acci);
          }
        }
        bool corr = false;
        if constexpr (F6) {
          corr = (w & 4096) != 0;
          if (__any(mine && corr)) {
            if (mine && corr) {
              ShortCorr cc;
              cc.dj0 = a.di0 + (double)seg.j;
              cc.step = a.step; cc.t0 = a.t0; cc.last = a.last; cc.dlast = a.dlast;
              short_op_corr<R, CPLX>(rc, opp, w, kf, cc, acc, acci);
            }
          }
        }
        if (mine && !chirp && !bare && !corr) {
#ifndef WFK_SH_SKIP0
#define WFK_SH_SKIP0 0
#endif
          if (cubic) short_op<R, true, CPLX, (F1 || WFK_SH_SKIP0)>(rc, opp, w, kf, a.step, acc, acci);
          else short_op<R, false, CPLX, (F1 || WFK_SH_SKIP0)>(rc, opp, w, kf, a.step, acc, acci);
        }
        if constexpr (F1)
        if (__any(lv && closing)) {
          const bool own = F2 && (w & 128) != 0;      // envelope x carrier in one op: adds its own term
          if constexpr (F2) {
            if (__any(lv && closing && own)) {
              if (lv && closing && own && (CPLX || !(w & 8))) short_cmul<R, CPLX>(rc, a.pool, w, kf, acc, acci);
            }
          }
          const bool xch = F4 && (w & 1024) != 0;    // chirp multiplier (exponential / hyperbolic)
          if constexpr (F4) {
            if (__any(lv && closing && xch)) {
              if (lv && closing && xch) short_xchirpmul<R, CPLX>(rc, w, kf, acc, acci);
            }
          }
          const int kind = (own || xch) ? -1 : (w & 3);      // 0: erf edge; 1: shared Gaussian; 2: INTERP table, 3: mollifier (stateless multipliers)
          if constexpr (F1) {
            if (__any(lv && closing && kind == 1)) {
              if (lv && closing && kind == 1) short_envmul<R, CPLX>(rc, kf, acc, acci);
            }
          }
          if (__any(lv && closing && kind == 0)) {
            if (lv && closing && kind == 0) short_erfmul_run<R, CPLX>(rc, kf, seg.len, acc, acci);
          }
          if constexpr (F2) {
            if (__any(lv && closing && kind == 2)) {
              if (lv && closing && kind == 2) short_tabmul<R, CPLX>(rc, a.pool, kf, acc, acci);
            }
            if (__any(lv && closing && kind == 3)) {
              if (lv && closing && kind == 3) short_mollmul<R, CPLX>(rc, kf, acc, acci);
            }
          }
        }
        return lv && !(w & WFK_SH_LAST);
        }
      };
      live = eval(rec, op, live);
      while (__any(live)) {
        op += (op_word(rec) & 3) > 1 ? WFK_SH_OP3 : WFK_SH_OP1;
        if (live) rec = load_op(op);
        live = eval(rec, op, live);
      }
    }

    // the next unit's segment and first op record: in flight while this unit is staged and stored
    const Seg nseg = decode(nslot, nxt);
    first = load_op(nseg.rec);

    if (cur.nslots != 0) {
      __syncthreads();            // the previous unit's store phase is done with the staging array
      if (cur.gaps & 1) {
        if constexpr (DAC) {
          // (whole groups of the constant's code, the group before the unit's first code included: plain layout)
          const unsigned f2 = (unsigned)(uint16_t)fillv * 0x10001u;
          SH_EACH(2, h)
            if (8 * (lane + 64 * h) < dhead + ns) *reinterpret_cast<u32x4*>(s_out + 8 * (lane + 64 * h)) = u32x4{f2, f2, f2, f2};
          SH_END
        } else {
        const int f0 = sw ? swz(lane) : lane;
        SH_EACH(16, r)
          if (64 * r < ns) s_out[f0 + rs * r] = fillv;
        SH_END
        }
        __syncthreads();
      }
      // clip (evaluated pieces only: every slot is one), + offset
      if (cur.do_clip) {
        if constexpr (CPLX) {
          // np.clip of complex values: lexicographic against the real bounds (see clip_np_cplx in wfk_kernels.hip)
          SH_EACH(R, k)
            if (acc[k] < cur.clip_lo || (acc[k] == cur.clip_lo && acci[k] < 0.0)) { acc[k] = cur.clip_lo; acci[k] = 0.0; }
            if (acc[k] > cur.clip_hi || (acc[k] == cur.clip_hi && acci[k] > 0.0)) { acc[k] = cur.clip_hi; acci[k] = 0.0; }
          SH_END
        } else if constexpr (PK) {
          // (the double path clips the fp64 sum and rounds once; here the float sum is clipped against the bounds --
          //  np.clip semantics, NaN propagates)
          SH_EACH(R, k)
            float v = accp[k / 2][k % 2];
            v = v < (float)cur.clip_lo ? (float)cur.clip_lo : v;
            v = v > (float)cur.clip_hi ? (float)cur.clip_hi : v;
            accp[k / 2][k % 2] = v;
          SH_END
        } else {
          SH_EACH(R, k) acc[k] = clip_np(acc[k], cur.clip_lo, cur.clip_hi); SH_END
        }
      }
      if constexpr (DAC) {
        // the run's codes at dhead + o + k: the unit's groups of 8 are the array's (plain layout)
        const int len = seg.len;
        E* const b0 = s_out + dhead + seg.o;
        SH_EACH(R, k)
          if (k < len) {
            const double v = acc[k] + cur.offset;
            unsigned rails, isnan;
            b0[k] = dac_code(v, dgain, doffset, dk.lo, dk.hi, dk.shift, rails, isnan);
            if constexpr (COUNT) { cnt_rails += rails; cnt_nan += isnan; }
          }
        SH_END
      } else
      {
        // padded layout: element o + k lands at swz(o) + k + [k >= 16 - (o & 15)]: two bases, immediate offsets
        const int o = seg.o, len = seg.len;
        const int t = sw ? 16 - (o & 15) : 99;
        E* const b0 = s_out + (sw ? swz(o) : o);
        SH_EACH(R, k)
          if (k < len) {                      // (a masked LDS write needs no wait: the branch is cheap)
            E* const at = (k >= t ? b0 + 1 : b0) + k;
            double v;
            if constexpr (PK) v = (double)(accp[k / 2][k % 2] + (float)cur.offset);
            else v = acc[k] + cur.offset;
            if constexpr (CPLX) {
              E e;
              e.x = (T)v;
              e.y = (T)acci[k];
              *at = e;
            } else {
              *at = (T)v;
            }
          }
        SH_END
      }
      __syncthreads();
    }

    // store the unit's range: 64 consecutive samples per instruction, 16 masked rows in two batches of
    // eight.  The LDS reads are unconditional (row 0's index clamped: lanes before the unit read element
    // 0 and never store it); a pure-fill unit (a zero stretch: skipped _zero pieces, no clip,
    // waveforms/_waveform.pyx:160-163) stores `offset`.
    if constexpr (DAC) {
      // The unit's codes sit at [dhead, tot) of a grid of 16-byte groups that starts dhead codes before its first one
      // (a 16-byte boundary of the output).  A lane's offset is in range only for what it owns: the range check drops
      // the rest (-1: past every buffer).  Nothing is loaded from the output.
      const int tot = dhead + ns;
      const __amdgpu_buffer_rsrc_t ores = make_rsrc(orow - dhead, (unsigned)tot * 2u);
      const unsigned f2 = (unsigned)(uint16_t)fillv * 0x10001u;
      SH_EACH(2, h)
        const int g = lane + 64 * h;
        u32x4 v = u32x4{f2, f2, f2, f2};
        if (cur.nslots != 0) v = *reinterpret_cast<const u32x4*>(s_out + 8 * g);
        const bool whole = 8 * g >= dhead && 8 * g + 8 <= tot;
        buf_store<u32x4>(v, ores, whole ? 16 * g : -1);
      SH_END
      // first and last partial group, code by code: lanes 0-7 group 0, lanes 8-15 the last group (where it is another)
      const int glast = (tot - 1) >> 3;
      const bool part0 = dhead != 0 || tot < 8, part1 = glast > 0 && (tot & 7) != 0;
      const int idx = lane < 8 ? lane : 8 * glast + (lane - 8);
      const bool on = lane < 16 && (lane < 8 ? part0 : part1) && idx >= dhead && idx < tot;
      E e = fillv;
      if (cur.nslots != 0) e = s_out[on ? idx : 0];
      buf_store16(e, ores, on ? 2 * idx : -1);
      if constexpr (COUNT) {
        unsigned s_rails = 0, s_nan = 0;                     // [below | above << 16], [nan | samples of the runs << 16]
        if (cur.nslots != 0) {
          s_rails = wave_sum(cnt_rails);
          s_nan = wave_sum(cnt_nan + ((unsigned)seg.len << 16));
        }
        const unsigned nfill = (unsigned)ns - (s_nan >> 16);  // samples no run covers: the constant's code
        const unsigned mine = lane == 0 ? (s_rails & 0xffffu) + (fill_rails & 1u) * nfill
                            : lane == 1 ? (s_rails >> 16) + (fill_rails >> 16) * nfill
                                        : (s_nan & 0xffffu) + fill_nan * nfill;
        if (lane < 3 && mine != 0) atomicAdd(dk.counts + (int64_t)cur.ch * 3 + lane, (unsigned long long)mine);
      }
    } else {
    const __amdgpu_buffer_rsrc_t ores = make_rsrc(orow, (unsigned)ns * (unsigned)sizeof(E));
    const int b0off = l0 * (int)sizeof(E);                  // row 0: "negative" for the lanes before the unit
    const int b1off = (64 + l0) * (int)sizeof(E);           // rows >= 1: never negative
    SH_EACH(2, hb)
      E v[8];
      SH_EACH(8, rr)
        constexpr int r = hb * 8 + rr;
        v[rr] = fillv;
        if (cur.nslots != 0) v[rr] = s_out[r == 0 ? max(s0, 0) : s0 + rs * r];
      SH_END
      if constexpr (ACC) {
        SH_EACH(8, rr)
          constexpr int r = hb * 8 + rr;
          add_old<E, CPLX>(v[rr], buf_load<E>(ores, r == 0 ? b0off : b1off + 64 * (r - 1) * (int)sizeof(E)));
        SH_END
      }
      SH_EACH(8, rr)
        constexpr int r = hb * 8 + rr;
        buf_store<E>(v[rr], ores, r == 0 ? b0off : b1off + 64 * (r - 1) * (int)sizeof(E));
      SH_END
    SH_END
    }

    cur = nxt;
    nxt = nn;
    seg = nseg;
    if constexpr (DAC) { dgain = ngain; doffset = noffset; }
  }
