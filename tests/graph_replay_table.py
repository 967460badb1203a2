"""Which entries of include/wfk.h the graph-replay table launches (tests/test_gpu_graph_replay.py), per family of its
cases.  A plain module without device imports: tests/test_graph_replay_cpu.py holds the header against it on the host, so
an apply that gains the promise "allocates nothing and does not synchronise" cannot be left out of the table silently."""

ROWS_OF = {
    'sampler': ('wfk_plan_launch', ),
    'iir_shared': ('wfk_iir_apply', ),
    'iir_rows': ('wfk_iir_rows_apply', ),
    'sampled_iir': ('wfk_chain_iir_launch', ),
    'sampled_iir_rows': ('wfk_chain_iir_rows_launch', ),
    'sampled_fir': ('wfk_chain_launch', ),
    'fir': ('wfk_fir_apply', ),
    'shift': ('wfk_shift_rows_apply', ),
    'mix': ('wfk_mix_rows_apply', ),
    'dac': ('wfk_dac_rows_apply', ),
    'marker': ('wfk_marker_rows_apply', 'wfk_marker_rows_apply_codes'),
    'demod': ('wfk_demod_apply', ),
    'probe': ('wfk_boxprobe_apply', ),
    'chain': ('wfk_iir_apply', 'wfk_shift_rows_apply', 'wfk_mix_rows_apply', 'wfk_dac_rows_apply',
              'wfk_marker_rows_apply_codes'),
    # each in a child process of its own (tests/graph_replay_rocfft.py)
    'rocfft': ('wfk_fir_apply', 'wfk_spectral_rows_apply', 'wfk_extract_rows_apply', 'wfk_spectral_apply'),
}

# entries the header documents as NOT capturable (its "Graph capture" paragraph names them); they carry no promise
NOT_CAPTURABLE = ()
