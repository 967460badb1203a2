// wfk_iir_rows_store.inc -- the store section of the per-row IIR tile body, the expansion of IRW_STORE_INC for the
// kernels that write their rows as T (iir_rows_tile, iir_rows_sampled, iir_rows_short): the barrier after sweep 2, the
// tile out of LDS as whole lines, the barrier that frees the tile array.  Included as TEXT by wfk_iir_rows_body.inc,
// where its names are in scope (tile, tid, y, base, left).
    __syncthreads();
    if (left >= IRW_TILE) {
#pragma unroll
      for (int i = 0; i < IRW_RUN; ++i) {
        const int j = i * IRW_THREADS + tid;
        y[base + j] = tile[(j / IRW_RUN) * IRW_PITCH + (j % IRW_RUN)];
      }
    } else {
#pragma unroll
      for (int i = 0; i < IRW_RUN; ++i) {
        const int j = i * IRW_THREADS + tid;
        if (j < left) y[base + j] = tile[(j / IRW_RUN) * IRW_PITCH + (j % IRW_RUN)];
      }
    }
    __syncthreads();
