"""ctypes binding of libwfk_hip.so (include/wfk.h).

This is the only door from Python to the sampler.  There is no fallback: if the
shared library is missing it cannot be imported, and if no GPU is visible every
launch raises.  ctypes releases the GIL during calls.
"""
from __future__ import annotations

import ctypes as C
import importlib.util
import os

import numpy as np

from ._flatten import Program, wfk_grid, wfk_program

_HERE = os.path.dirname(os.path.abspath(__file__))
# WFK_LIB: developer knob for A/B builds of the same library (tools/*_bench.py)
LIB_PATH = os.environ.get('WFK_LIB') or os.path.join(_HERE, 'csrc', 'libwfk_hip.so')

OUT_F64, OUT_F32, OUT_C128, OUT_C64 = 0, 1, 2, 3
ACCUMULATE = 1
_KIND_OF = {np.dtype(np.float64): OUT_F64, np.dtype(np.float32): OUT_F32,
            np.dtype(np.complex128): OUT_C128, np.dtype(np.complex64): OUT_C64}
_DTYPE_OF = {v: k for k, v in _KIND_OF.items()}

E_UNSUP = -2
E_TIMEOUT = -5


class wfk_plan_info(C.Structure):
    _fields_ = [('n_channels', C.c_int32), ('n', C.c_int64), ('tile', C.c_int32),
                ('n_tiles', C.c_int64), ('n_pieces', C.c_int32),
                ('param_doubles', C.c_int64), ('n_fast', C.c_int32),
                ('n_direct', C.c_int32), ('n_fused', C.c_int32),
                ('n_generic', C.c_int32)]


class EngineError(RuntimeError):
    pass


_lib = None


def lib():
    """Load libwfk_hip.so (built by waveforms_amd/csrc/Makefile or
    __graft_entry__.build()).  Fails loudly when it is absent."""
    global _lib
    if _lib is None:
        if not os.path.exists(LIB_PATH):
            raise EngineError(
                f'{LIB_PATH} not found: build it with `make -C waveforms_amd/csrc` '
                f'(hipcc --offload-arch=gfx950). waveforms_amd has no CPU sampling path.')
        # PyTorch wheels bundle their own libamdhip64 / libhsa-runtime64 / librocfft under
        # the same SONAMEs as /opt/rocm.  Whichever is loaded first serves the whole
        # process, and a system runtime loaded before torch leaves torch without a GPU.
        # So when torch is installed, let it load its runtime first.
        if importlib.util.find_spec('torch') is not None:
            import torch  # noqa: F401
        l = C.CDLL(LIB_PATH)
        l.wfk_last_error.restype = C.c_char_p
        P, I64, I32, VP = C.POINTER, C.c_int64, C.c_int32, C.c_void_p
        l.wfk_plan_create_grid.argtypes = [P(wfk_program), P(wfk_grid), P(VP)]
        l.wfk_plan_create_tlist.argtypes = [P(wfk_program), VP, I64, P(VP)]
        l.wfk_grid_detect.argtypes = [VP, I64, P(wfk_grid)]
        l.wfk_grid_detect_runs.argtypes = [VP, I64, I64, I32, VP, P(wfk_grid)]
        l.wfk_plan_destroy.argtypes = [VP]
        l.wfk_plan_get_info.argtypes = [VP, P(wfk_plan_info)]
        l.wfk_plan_member_index.argtypes = [VP, I32, VP, I32]
        l.wfk_plan_channel_is_complex.argtypes = [VP, I32]
        l.wfk_plan_kernel_name.argtypes = [VP, C.c_int]
        l.wfk_plan_kernel_name.restype = C.c_char_p
        l.wfk_plan_table_bytes.argtypes = [VP]
        l.wfk_plan_table_bytes.restype = C.c_int64
        l.wfk_plan_launch.argtypes = [VP, VP, I64, C.c_int, C.c_uint32, VP]
        l.wfk_plan_run_host.argtypes = [VP, VP, I64, C.c_int]
        l.wfk_fir_plan_create.argtypes = [VP, I32, I64, I32, C.c_int, P(VP)]
        l.wfk_fir_plan_create_rows.argtypes = [VP, I32, I64, I32, C.c_int, P(VP)]
        l.wfk_chain_plan_create_rows.argtypes = [P(wfk_program), P(wfk_grid), VP, I32, C.c_int, P(VP)]
        l.wfk_fir_apply.argtypes = [VP, VP, I64, VP, I64, VP]
        l.wfk_fir_plan_destroy.argtypes = [VP]
        l.wfk_fir_kernel_name.argtypes = [VP]
        l.wfk_fir_kernel_name.restype = C.c_char_p
        l.wfk_chain_plan_create.argtypes = [P(wfk_program), P(wfk_grid), VP, I32, C.c_int, P(VP)]
        l.wfk_chain_is_fused.argtypes = [VP]
        l.wfk_chain_unfused_reason.argtypes = [VP]
        l.wfk_chain_unfused_reason.restype = C.c_char_p
        l.wfk_chain_kernel_name.argtypes = [VP]
        l.wfk_chain_kernel_name.restype = C.c_char_p
        l.wfk_chain_table_bytes.argtypes = [VP]
        l.wfk_chain_table_bytes.restype = I64
        l.wfk_chain_launch.argtypes = [VP, VP, I64, VP]
        l.wfk_chain_plan_destroy.argtypes = [VP]
        l.wfk_chain_iir_plan_create.argtypes = [P(wfk_program), P(wfk_grid), I32, VP, VP, VP, VP, I32, I32, C.c_int, P(VP)]
        l.wfk_chain_iir_is_fused.argtypes = [VP]
        l.wfk_chain_iir_unfused_reason.argtypes = [VP]
        l.wfk_chain_iir_unfused_reason.restype = C.c_char_p
        l.wfk_chain_iir_kernel_name.argtypes = [VP]
        l.wfk_chain_iir_kernel_name.restype = C.c_char_p
        l.wfk_chain_iir_table_bytes.argtypes = [VP]
        l.wfk_chain_iir_table_bytes.restype = I64
        l.wfk_chain_iir_state_dim.argtypes = [VP]
        l.wfk_chain_iir_launch.argtypes = [VP, VP, I64, VP, VP, C.c_double, VP]
        l.wfk_chain_iir_status.argtypes = [VP, VP]
        l.wfk_chain_iir_plan_destroy.argtypes = [VP]
        l.wfk_chain_iir_rows_plan_create.argtypes = [P(wfk_program), P(wfk_grid), I32, VP, VP, VP, C.c_int, P(VP)]
        l.wfk_chain_iir_rows_is_fused.argtypes = [VP]
        l.wfk_chain_iir_rows_unfused_reason.argtypes = [VP]
        l.wfk_chain_iir_rows_unfused_reason.restype = C.c_char_p
        l.wfk_chain_iir_rows_kernel_name.argtypes = [VP]
        l.wfk_chain_iir_rows_kernel_name.restype = C.c_char_p
        l.wfk_chain_iir_rows_table_bytes.argtypes = [VP]
        l.wfk_chain_iir_rows_table_bytes.restype = I64
        l.wfk_chain_iir_rows_state_dim.argtypes = [VP]
        l.wfk_chain_iir_rows_launch.argtypes = [VP, VP, I64, VP, VP, VP, VP]
        l.wfk_chain_iir_rows_plan_destroy.argtypes = [VP]
        l.wfk_iir_plan_create.argtypes = [I32, VP, VP, VP, I64, I32, C.c_int, P(VP)]
        l.wfk_iir_state_dim.argtypes = [VP]
        l.wfk_iir_apply.argtypes = [VP, VP, I64, VP, I64, VP, VP, C.c_double, VP]
        l.wfk_iir_plan_destroy.argtypes = [VP]
        l.wfk_iir_status.argtypes = [VP, VP]
        l.wfk_iir_kernel_name.argtypes = [VP]
        l.wfk_iir_kernel_name.restype = C.c_char_p
        l.wfk_iir_rows_plan_create.argtypes = [I32, VP, VP, VP, I64, I32, C.c_int, P(VP)]
        l.wfk_iir_rows_state_dim.argtypes = [VP]
        l.wfk_iir_rows_apply.argtypes = [VP, VP, I64, VP, I64, VP, VP, VP, VP]
        l.wfk_iir_rows_apply_shared_in.argtypes = [VP, VP, VP, I64, VP, VP, VP, VP]
        l.wfk_iir_rows_kernel_name.argtypes = [VP]
        l.wfk_iir_rows_kernel_name.restype = C.c_char_p
        l.wfk_iir_rows_plan_destroy.argtypes = [VP]
        l.wfk_spectral_plan_create.argtypes = [I64, I32, C.c_int, P(VP)]
        l.wfk_spectral_apply.argtypes = [VP, VP, VP, VP, VP]
        l.wfk_spectral_plan_destroy.argtypes = [VP]
        l.wfk_spectral_rows_plan_create.argtypes = [I64, I32, C.c_int, C.c_double, VP, VP, P(VP)]
        l.wfk_spectral_rows_apply.argtypes = [VP, VP, I64, VP, I64, VP]
        l.wfk_spectral_rows_plan_destroy.argtypes = [VP]
        l.wfk_spectral_rows_phase_step.argtypes = [C.c_double, C.c_double, I64, P(C.c_double), P(C.c_double)]
        l.wfk_shift_rows_plan_create.argtypes = [I64, I32, C.c_int, VP, VP, P(VP)]
        l.wfk_shift_rows_apply.argtypes = [VP, VP, I64, VP, I64, VP]
        l.wfk_shift_rows_kernel_name.argtypes = [VP]
        l.wfk_shift_rows_kernel_name.restype = C.c_char_p
        l.wfk_shift_rows_plan_destroy.argtypes = [VP]
        l.wfk_dac_rows_plan_create.argtypes = [I64, I32, C.c_int, VP, VP, C.c_int, C.c_int, C.c_int, P(VP)]
        l.wfk_dac_rows_apply.argtypes = [VP, VP, I64, VP, I64, VP, VP]
        l.wfk_dac_rows_kernel_name.argtypes = [VP, C.c_int]
        l.wfk_dac_rows_kernel_name.restype = C.c_char_p
        l.wfk_dac_rows_plan_destroy.argtypes = [VP]
        l.wfk_iir_rows_dac_plan_create.argtypes = [I32, VP, VP, VP, I64, I32, C.c_int, VP, VP, C.c_int, C.c_int, P(VP)]
        l.wfk_iir_rows_dac_state_dim.argtypes = [VP]
        l.wfk_iir_rows_dac_apply.argtypes = [VP, VP, I64, VP, I64, VP, VP, VP, VP, VP]
        l.wfk_iir_rows_dac_apply_shared_in.argtypes = [VP, VP, VP, I64, VP, VP, VP, VP, VP]
        l.wfk_iir_rows_dac_kernel_name.argtypes = [VP]
        l.wfk_iir_rows_dac_kernel_name.restype = C.c_char_p
        l.wfk_iir_rows_dac_plan_destroy.argtypes = [VP]
        l.wfk_chain_iir_rows_dac_plan_create.argtypes = [P(wfk_program), P(wfk_grid), I32, VP, VP, VP, VP, VP, C.c_int,
                                                         C.c_int, P(VP)]
        l.wfk_chain_iir_rows_dac_is_fused.argtypes = [VP]
        l.wfk_chain_iir_rows_dac_unfused_reason.argtypes = [VP]
        l.wfk_chain_iir_rows_dac_unfused_reason.restype = C.c_char_p
        l.wfk_chain_iir_rows_dac_kernel_name.argtypes = [VP]
        l.wfk_chain_iir_rows_dac_kernel_name.restype = C.c_char_p
        l.wfk_chain_iir_rows_dac_table_bytes.argtypes = [VP]
        l.wfk_chain_iir_rows_dac_table_bytes.restype = I64
        l.wfk_chain_iir_rows_dac_state_dim.argtypes = [VP]
        l.wfk_chain_iir_rows_dac_launch.argtypes = [VP, VP, I64, VP, VP, I64, VP, VP, VP, VP]
        l.wfk_chain_iir_rows_dac_plan_destroy.argtypes = [VP]
        l.wfk_chain_dac_plan_create.argtypes = [P(wfk_program), P(wfk_grid), VP, VP, C.c_int, C.c_int, C.c_int, P(VP)]
        l.wfk_chain_dac_is_fused.argtypes = [VP]
        l.wfk_chain_dac_unfused_reason.argtypes = [VP]
        l.wfk_chain_dac_unfused_reason.restype = C.c_char_p
        l.wfk_chain_dac_kernel_name.argtypes = [VP, C.c_int]
        l.wfk_chain_dac_kernel_name.restype = C.c_char_p
        l.wfk_chain_dac_table_bytes.argtypes = [VP]
        l.wfk_chain_dac_table_bytes.restype = I64
        l.wfk_chain_dac_launch.argtypes = [VP, VP, I64, VP, VP, I64, VP]
        l.wfk_chain_dac_plan_destroy.argtypes = [VP]
        l.wfk_marker_rows_plan_create.argtypes = [I64, I32, C.c_int, C.c_int, VP, VP, VP, P(VP)]
        l.wfk_marker_rows_apply.argtypes = [VP, VP, I64, VP, I64, VP, VP]
        l.wfk_marker_rows_apply_codes.argtypes = [VP, VP, I64, VP, I64, C.c_int, VP, VP]
        l.wfk_marker_rows_span.argtypes = [VP, C.c_int]
        l.wfk_marker_rows_span.restype = I64
        l.wfk_marker_rows_kernel_name.argtypes = [VP, C.c_int, C.c_int]
        l.wfk_marker_rows_kernel_name.restype = C.c_char_p
        l.wfk_marker_rows_plan_destroy.argtypes = [VP]
        l.wfk_segment_rows_plan_create.argtypes = [I64, I32, C.c_int, I64, I64, I64, P(VP)]
        l.wfk_segment_rows_apply_bit.argtypes = [VP, VP, I64, C.c_int, VP, I64, VP, I64, VP, VP]
        l.wfk_segment_rows_apply_marks.argtypes = [VP, VP, I64, VP, I64, VP, I64, VP, I64, VP, VP]
        l.wfk_segment_rows_span.argtypes = [VP]
        l.wfk_segment_rows_span.restype = I64
        l.wfk_segment_rows_kernel_name.argtypes = [VP, C.c_int, C.c_int]
        l.wfk_segment_rows_kernel_name.restype = C.c_char_p
        l.wfk_segment_rows_plan_destroy.argtypes = [VP]
        l.wfk_segment_library_plan_create.argtypes = [I32, C.c_int, I64, I64, I64, P(VP)]
        l.wfk_segment_library_apply.argtypes = [VP, VP, I64, VP, I64, VP, VP, I64, VP, I64, VP, I64, VP, VP]
        l.wfk_segment_library_kernel_name.argtypes = [VP, C.c_int]
        l.wfk_segment_library_kernel_name.restype = C.c_char_p
        l.wfk_segment_library_plan_destroy.argtypes = [VP]
        l.wfk_segment_play_plan_create.argtypes = [I64, I32, C.c_int, I64, I64, P(VP)]
        l.wfk_segment_play_apply.argtypes = [VP, VP, I64, VP, I64, VP, C.c_int16, C.c_int16, VP, I64, VP, I64, VP, VP]
        l.wfk_segment_play_span.argtypes = [VP]
        l.wfk_segment_play_span.restype = I64
        l.wfk_segment_play_kernel_name.argtypes = [VP, C.c_int]
        l.wfk_segment_play_kernel_name.restype = C.c_char_p
        l.wfk_segment_play_plan_destroy.argtypes = [VP]
        l.wfk_mix_rows_plan_create.argtypes = [I64, I32, I32, C.c_int, VP, VP, VP, VP, P(VP)]
        l.wfk_mix_rows_apply.argtypes = [VP, VP, I64, VP, I64, VP]
        l.wfk_mix_rows_reads.argtypes = [VP]
        l.wfk_mix_rows_reads.restype = I64
        l.wfk_mix_rows_kernel_name.argtypes = [VP]
        l.wfk_mix_rows_kernel_name.restype = C.c_char_p
        l.wfk_mix_rows_plan_destroy.argtypes = [VP]
        l.wfk_mix_dac_plan_create.argtypes = [I64, I32, I32, C.c_int, VP, VP, VP, VP, VP, VP, C.c_int, C.c_int, C.c_int,
                                              P(VP)]
        l.wfk_mix_dac_apply.argtypes = [VP, VP, I64, VP, I64, VP, VP]
        l.wfk_mix_dac_reads.argtypes = [VP]
        l.wfk_mix_dac_reads.restype = I64
        l.wfk_mix_dac_span.argtypes = [VP]
        l.wfk_mix_dac_span.restype = I64
        l.wfk_mix_dac_kernel_name.argtypes = [VP, C.c_int]
        l.wfk_mix_dac_kernel_name.restype = C.c_char_p
        l.wfk_mix_dac_plan_destroy.argtypes = [VP]
        l.wfk_curve_rows_plan_create.argtypes = [I64, I32, C.c_int, VP, VP, VP, VP, VP, P(VP)]
        l.wfk_curve_rows_apply.argtypes = [VP, VP, I64, VP, I64, VP, VP]
        l.wfk_curve_rows_spans.argtypes = [VP]
        l.wfk_curve_rows_kernel_name.argtypes = [VP, C.c_int]
        l.wfk_curve_rows_kernel_name.restype = C.c_char_p
        l.wfk_curve_rows_plan_destroy.argtypes = [VP]
        l.wfk_curve_iir_dac_plan_create.argtypes = [I32, VP, VP, VP, I64, I32, C.c_int, VP, VP, VP, VP, VP, VP, VP,
                                                    C.c_int, C.c_int, P(VP)]
        l.wfk_curve_iir_dac_state_dim.argtypes = [VP]
        l.wfk_curve_iir_dac_apply.argtypes = [VP, VP, I64, VP, I64, VP, VP, VP, VP, VP, VP]
        l.wfk_curve_iir_dac_apply_shared_in.argtypes = [VP, VP, VP, I64, VP, VP, VP, VP, VP, VP]
        l.wfk_curve_iir_dac_kernel_name.argtypes = [VP]
        l.wfk_curve_iir_dac_kernel_name.restype = C.c_char_p
        l.wfk_curve_iir_dac_plan_destroy.argtypes = [VP]
        l.wfk_chain_curve_iir_dac_plan_create.argtypes = [P(wfk_program), P(wfk_grid), I32, VP, VP, VP, VP, VP, VP, VP,
                                                          VP, VP, VP, C.c_int, C.c_int, P(VP)]
        l.wfk_chain_curve_iir_dac_is_fused.argtypes = [VP]
        l.wfk_chain_curve_iir_dac_unfused_reason.argtypes = [VP]
        l.wfk_chain_curve_iir_dac_unfused_reason.restype = C.c_char_p
        l.wfk_chain_curve_iir_dac_kernel_name.argtypes = [VP]
        l.wfk_chain_curve_iir_dac_kernel_name.restype = C.c_char_p
        l.wfk_chain_curve_iir_dac_table_bytes.argtypes = [VP]
        l.wfk_chain_curve_iir_dac_table_bytes.restype = I64
        l.wfk_chain_curve_iir_dac_state_dim.argtypes = [VP]
        l.wfk_chain_curve_iir_dac_launch.argtypes = [VP, VP, I64, VP, VP, VP, I64, VP, VP, VP, VP]
        l.wfk_chain_curve_iir_dac_plan_destroy.argtypes = [VP]
        l.wfk_extract_rows_plan_create.argtypes = [I64, I32, I32, VP, I32, I64, P(VP)]
        l.wfk_extract_rows_apply.argtypes = [VP, VP, I64, VP, I64, VP, I64, VP]
        l.wfk_extract_rows_kernel_name.argtypes = [VP]
        l.wfk_extract_rows_kernel_name.restype = C.c_char_p
        l.wfk_extract_rows_plan_destroy.argtypes = [VP]
        l.wfk_demod_plan_create.argtypes = [VP, I64, I32, C.c_int, P(VP)]
        l.wfk_demod_apply.argtypes = [VP, VP, I64, I64, VP, I64, VP]
        l.wfk_demod_kernel_name.argtypes = [VP, I64]
        l.wfk_demod_kernel_name.restype = C.c_char_p
        l.wfk_demod_plan_destroy.argtypes = [VP]
        l.wfk_bdemod_plan_create.argtypes = [VP, I64, I32, C.c_int, I64, I64, I64, P(VP)]
        l.wfk_bdemod_apply.argtypes = [VP, VP, I64, I64, VP, I64, VP]
        l.wfk_bdemod_bin_groups.argtypes = [I64, I32, I64]
        l.wfk_bdemod_bin_groups.restype = I64
        l.wfk_bdemod_kernel_name.argtypes = [VP, I64]
        l.wfk_bdemod_kernel_name.restype = C.c_char_p
        l.wfk_bdemod_plan_destroy.argtypes = [VP]
        l.wfk_avg_plan_create.argtypes = [I64, I64, C.c_int, P(VP)]
        l.wfk_avg_apply.argtypes = [VP, VP, I64, I64, I64, VP, I64, VP, I64, C.c_int, VP]
        l.wfk_avg_splits.argtypes = [VP, I64, I64]
        l.wfk_avg_splits.restype = I64
        l.wfk_avg_kernel_name.argtypes = [VP, I64, C.c_int]
        l.wfk_avg_kernel_name.restype = C.c_char_p
        l.wfk_avg_plan_destroy.argtypes = [VP]
        l.wfk_states_plan_create.argtypes = [VP, I32, I32, I64, P(VP)]
        l.wfk_states_apply.argtypes = [VP, VP, I64, I64, I64, VP, I64, VP, VP, VP, C.c_int, VP]
        l.wfk_states_kernel_name.argtypes = [VP, I64]
        l.wfk_states_kernel_name.restype = C.c_char_p
        l.wfk_states_plan_destroy.argtypes = [VP]
        l.wfk_boxprobe_brackets.argtypes = [VP, I64, VP, I64, VP, VP, VP]
        l.wfk_boxprobe_plan_create.argtypes = [VP, I64, VP, I32, I64, I64, C.c_double, P(VP)]
        l.wfk_boxprobe_apply.argtypes = [VP, VP, I64, I64, VP, I64, VP]
        l.wfk_boxprobe_kernel_name.argtypes = [VP]
        l.wfk_boxprobe_kernel_name.restype = C.c_char_p
        l.wfk_boxprobe_plan_destroy.argtypes = [VP]
        l.wfk_host_alloc.argtypes = [P(VP), C.c_size_t]
        l.wfk_host_free.argtypes = [VP]
        l.wfk_host_all_finite.argtypes = [VP, I64]
        l.wfk_malloc.argtypes = [P(VP), C.c_size_t]
        l.wfk_free.argtypes = [VP]
        l.wfk_memcpy_h2d.argtypes = [VP, VP, C.c_size_t]
        l.wfk_memcpy_d2h.argtypes = [VP, VP, C.c_size_t]
        l.wfk_memset.argtypes = [VP, C.c_int, C.c_size_t]
        l.wfk_stream_sync.argtypes = [VP]
        l.wfk_device_count.argtypes = [P(C.c_int)]
        l.wfk_set_device.argtypes = [C.c_int]
        if l.wfk_abi_version() != 2:
            raise EngineError('libwfk_hip.so ABI version mismatch')
        _lib = l
    return _lib


def check(rc):
    if rc < 0:
        msg = lib().wfk_last_error().decode('utf-8', 'replace')
        if rc == E_UNSUP:
            raise NotImplementedError(msg)
        raise EngineError(f'wfk error {rc}: {msg}')
    return rc


def device_count() -> int:
    n = C.c_int(0)
    rc = lib().wfk_device_count(C.byref(n))
    return n.value if rc == 0 else 0


def set_device(ordinal: int):
    check(lib().wfk_set_device(ordinal))


def detect_grid(t: np.ndarray):
    """-> wfk_grid if the float64 array `t` is bit-identical to a np.linspace / np.arange grid
    (exact element-wise check inside the library), else None."""
    if os.environ.get('WFK_NO_GRID_DETECT') == '1' or t.dtype != np.float64 or not t.flags.c_contiguous:
        return None
    g = wfk_grid()
    return g if lib().wfk_grid_detect(t.ctypes.data, len(t), C.byref(g)) == 1 else None


def detect_grid_runs(t: np.ndarray, min_len: int = 4096, max_runs: int = 256):
    """-> [(start, wfk_grid), ...] if the float64 array `t` is several NumPy grids back to back (each run
    verified element by element, at least `min_len` samples long), else None."""
    if os.environ.get('WFK_NO_GRID_DETECT') == '1' or t.dtype != np.float64 or not t.flags.c_contiguous:
        return None
    starts = np.zeros(max_runs, dtype=np.int64)
    grids = (wfk_grid * max_runs)()
    k = lib().wfk_grid_detect_runs(t.ctypes.data, len(t), min_len, max_runs, starts.ctypes.data, grids)
    if k <= 0:
        return None
    out = []
    for i in range(k):
        g = wfk_grid()
        C.memmove(C.byref(g), C.byref(grids[i]), C.sizeof(wfk_grid))
        out.append((int(starts[i]), g))
    return out


class _Handle:
    """Owner of one library handle: `_h` is there from the first moment of the object's life (so `close` and `__del__`
    are safe on an object whose constructor raised), `_destroy` names the library function that releases it."""
    _destroy = None

    def __new__(cls, *args, **kwargs):
        self = super().__new__(cls)
        self._h = C.c_void_p()
        return self

    def close(self):
        if self._h and _lib is not None:      # (_lib is None once the interpreter takes the module down)
            getattr(_lib, self._destroy)(self._h)
            self._h = C.c_void_p()

    __del__ = close

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()


class Plan(_Handle):
    """A compiled program bound to a time axis (grid or explicit t)."""
    _destroy = 'wfk_plan_destroy'

    def __init__(self, prog: Program, grid: wfk_grid | None = None, t=None):
        self.prog = prog
        if grid is not None:
            self.grid = grid
            check(lib().wfk_plan_create_grid(C.byref(prog.struct), C.byref(grid),
                                             C.byref(self._h)))
        else:
            t = np.ascontiguousarray(t, dtype=np.float64)
            check(lib().wfk_plan_create_tlist(C.byref(prog.struct), t.ctypes.data,
                                              len(t), C.byref(self._h)))
        info = wfk_plan_info()
        check(lib().wfk_plan_get_info(self._h, C.byref(info)))
        self.info = info
        self.n = int(info.n)
        self.n_channels = int(info.n_channels)

    def member_index(self, member: int) -> np.ndarray:
        """np.searchsorted(x - shift, bounds) of one member, computed by the library."""
        nb = len(self.prog.member_bounds(member))
        idx = np.empty(nb, dtype=np.int64)
        check(lib().wfk_plan_member_index(self._h, member, idx.ctypes.data, nb))
        return idx

    def kernel_name(self, dtype=np.float64) -> str:
        """Symbol of the kernel a launch with this output dtype runs (as rocprofv3 shows it)."""
        return lib().wfk_plan_kernel_name(self._h, _KIND_OF[np.dtype(dtype)]).decode()

    def table_bytes(self) -> int:
        """Bytes of device tables a launch reads next to the output stream."""
        return int(lib().wfk_plan_table_bytes(self._h))

    def launch(self, out_ptr: int, ch_stride: int, kind: int, accumulate=False,
               stream: int = 0):
        """Asynchronous launch into device memory at `out_ptr`."""
        check(lib().wfk_plan_launch(self._h, out_ptr, ch_stride, kind,
                                    ACCUMULATE if accumulate else 0, stream))

    def run_host(self, dtype=np.float64) -> np.ndarray:
        """Launch, copy back, synchronise -> (n_channels, n) NumPy array.  Big results live in a
        page-locked block from the library's cache (`pinned_empty`): no page faults, DMA straight into
        it, and for a single channel the copy overlaps the kernel part by part."""
        dtype = np.dtype(dtype)
        out = pinned_empty((self.n_channels, self.n), dtype)
        if out.size:
            check(lib().wfk_plan_run_host(self._h, out.ctypes.data, self.n,
                                          _KIND_OF[dtype]))
        return out

    def run_host_into(self, out: np.ndarray):
        """Launch and copy straight into the caller's C-contiguous array of n_channels * n elements
        (`Waveform.__call__(x, out=...)`): no temporary, no second pass over the data."""
        if out.size != self.n_channels * self.n or not out.flags.c_contiguous or not out.flags.writeable:
            raise ValueError('out must be a writeable C-contiguous array of n_channels * n elements')
        if out.size:
            check(lib().wfk_plan_run_host(self._h, out.ctypes.data, self.n, _KIND_OF[out.dtype]))
        return out


PINNED_MIN_BYTES = 4 << 20


def all_finite(a: np.ndarray) -> bool:
    """no NaN / inf in a C-contiguous float64 / complex128 array (threaded scan inside the library)"""
    n = a.size * (2 if a.dtype == np.complex128 else 1)
    return bool(lib().wfk_host_all_finite(a.ctypes.data, n))


def pinned_empty(shape, dtype) -> np.ndarray:
    """np.empty, but results of >= 4 MB are backed by a page-locked block from the library's cache
    (wfk_host_alloc); the block goes back to the cache when the array and all its views are gone.
    Falls back to an ordinary array when pinned memory is not to be had."""
    import weakref
    dtype = np.dtype(dtype)
    nbytes = int(np.prod(shape)) * dtype.itemsize
    if nbytes < PINNED_MIN_BYTES:
        return np.empty(shape, dtype=dtype)
    p = C.c_void_p()
    if lib().wfk_host_alloc(C.byref(p), nbytes) != 0 or not p.value:
        return np.empty(shape, dtype=dtype)
    buf = (C.c_byte * nbytes).from_address(p.value)
    weakref.finalize(buf, lib().wfk_host_free, p.value)
    return np.frombuffer(buf, dtype=dtype).reshape(shape)


class FirPlan(_Handle):
    """out[i] = sum_k ker[k] * sig[i + K//2 - k] (zero padded) for `batch` rows.  A 2-D `ker` of shape
    (batch, K) gives every row its own kernel (one predistortion kernel per AWG line)."""
    _destroy = 'wfk_fir_plan_destroy'

    def __init__(self, ker, n: int, batch: int = 1, dtype=np.float64):
        ker = np.ascontiguousarray(ker, dtype=np.float64)
        self.n, self.batch, self.dtype = int(n), int(batch), np.dtype(dtype)
        if ker.ndim == 2:
            if ker.shape[0] != self.batch:
                raise ValueError('per-row kernels: ker must have shape (batch, K)')
            check(lib().wfk_fir_plan_create_rows(ker.ctypes.data, ker.shape[1], self.n, self.batch,
                                                 _KIND_OF[self.dtype], C.byref(self._h)))
        else:
            check(lib().wfk_fir_plan_create(ker.ctypes.data, len(ker), self.n, self.batch,
                                            _KIND_OF[self.dtype], C.byref(self._h)))

    def apply(self, in_ptr: int, in_stride: int, out_ptr: int, out_stride: int,
              stream: int = 0):
        check(lib().wfk_fir_apply(self._h, in_ptr, in_stride, out_ptr, out_stride,
                                  stream))

    def kernel_name(self) -> str:
        """'fir_fused<T>' (+ ' x N' accumulated passes, + ' per-row spectra') or
        'fir_gather<T> + rocfft<L=..,rows=..> + fir_multiply<T> + fir_scatter<T>'"""
        return lib().wfk_fir_kernel_name(self._h).decode()


class ChainPlan(_Handle):
    """sampler -> FIR for every channel of `prog` on `grid` (predistort(wav(t), ker=ker)); fused
    into ONE kernel when the program is fully fused (lean plan on a fine grid, or a pure short-tier
    plan at AWG sample rates) and K <= 1537 (`fused`, `why_not`, `kernel_name()`)."""
    _destroy = 'wfk_chain_plan_destroy'

    def __init__(self, prog: Program, grid: wfk_grid, ker, dtype=np.float64):
        ker = np.ascontiguousarray(ker, dtype=np.float64)
        self.prog, self.grid, self.dtype = prog, grid, np.dtype(dtype)
        self.n, self.n_channels = int(grid.n), prog.n_channels
        if ker.ndim == 2:          # one kernel per channel
            if ker.shape[0] != prog.n_channels:
                raise ValueError('per-channel kernels: ker must have shape (n_channels, K)')
            check(lib().wfk_chain_plan_create_rows(C.byref(prog.struct), C.byref(grid), ker.ctypes.data, ker.shape[1],
                                                   _KIND_OF[self.dtype], C.byref(self._h)))
        else:
            check(lib().wfk_chain_plan_create(C.byref(prog.struct), C.byref(grid), ker.ctypes.data, len(ker),
                                              _KIND_OF[self.dtype], C.byref(self._h)))
        self.fused = bool(lib().wfk_chain_is_fused(self._h))
        self.why_not = lib().wfk_chain_unfused_reason(self._h).decode()

    def launch(self, out_ptr: int, out_stride: int, stream: int = 0):
        check(lib().wfk_chain_launch(self._h, out_ptr, out_stride, stream))

    def kernel_name(self) -> str:
        """'fir_sampled<T,HOPB>' (fine grids), 'fir_short<T,HOPB>' (AWG rates) or the unfused pair"""
        return lib().wfk_chain_kernel_name(self._h).decode()

    def table_bytes(self) -> int:
        return int(lib().wfk_chain_table_bytes(self._h))


def _accepted(rc) -> bool:
    """An IIR launch / status code: False for WFK_ETIMEOUT (a look-back timed out; the plan has switched to the
    three-launch form), True for success; any other error raises"""
    if rc == E_TIMEOUT:
        return False
    check(rc)
    return True


def iir_run_checked(launch, status, retry=True) -> bool:
    """The synchronous form of the look-back protocol, spelt once: `launch()` (-> False: refused after an earlier
    timeout), then `status()` (synchronises; -> False: a look-back of this launch timed out, the outputs hold NaN);
    after a failure the plan runs in the three-launch form, so launch and check once more -- unless `retry` is
    False (an in-place pass: the input is gone).  -> whether the outputs are good; the caller raises its own error."""
    def attempt():
        ok = launch()
        return status() and ok
    return attempt() or (retry and attempt())


def sos_sections(sos):
    """an SOS matrix (scipy.signal.sosfilt) -> [(b, a), ...]"""
    return [(row[:3], row[3:]) for row in np.asarray(sos, dtype=np.float64).reshape(-1, 6)]


def _pack_sections(sections):
    """list of (b, a) -> (orders int32, b flat, a flat), every section padded to max(len(b), len(a))"""
    orders, bs, as_ = [], [], []
    for b, a in sections:
        b = np.atleast_1d(np.asarray(b, dtype=np.float64))
        a = np.atleast_1d(np.asarray(a, dtype=np.float64))
        m = max(len(b), len(a))
        bs.append(np.concatenate([b, np.zeros(m - len(b))]))
        as_.append(np.concatenate([a, np.zeros(m - len(a))]))
        orders.append(m - 1)
    return (np.asarray(orders, dtype=np.int32), np.ascontiguousarray(np.concatenate(bs)),
            np.ascontiguousarray(np.concatenate(as_)))


class ChainIirPlan(_Handle):
    """sampler -> IIR cascade (-> FIR) for every channel of `prog` on `grid`, device-resident:
    `sosfilt(sos, wav(t) - initial, zi) + initial` of Waveform.sample(filters=) (reference waveform.py:190-203,
    244-251) and `predistort(wav(t), filters, ker)` (distortion.py:298-337).  When the program is fully fused and the
    (first pass of the) cascade has a state dimension <= 4, the wave that owns a chunk of the IIR scan EVALUATES its
    input (`iir_sampled<...>`): the unfiltered samples never touch HBM (`fused`, `why_not`, `kernel_name()`).
    `ker` (K,) or (n_channels, K): an FIR stage behind the cascade."""
    _destroy = 'wfk_chain_iir_plan_destroy'

    def __init__(self, prog: Program, grid: wfk_grid, sections, ker=None, dtype=np.float64):
        orders, bflat, aflat = _pack_sections(sections)
        self.prog, self.grid, self.dtype = prog, grid, np.dtype(dtype)
        self.n, self.n_channels = int(grid.n), prog.n_channels
        kp, K, rows = None, 0, 0
        if ker is not None:
            ker = np.ascontiguousarray(ker, dtype=np.float64)
            if ker.ndim == 2 and ker.shape[0] != prog.n_channels:
                raise ValueError('per-channel kernels: ker must have shape (n_channels, K)')
            kp, K, rows = ker.ctypes.data, ker.shape[-1], int(ker.ndim == 2)
        check(lib().wfk_chain_iir_plan_create(C.byref(prog.struct), C.byref(grid), len(orders), orders.ctypes.data,
                                              bflat.ctypes.data, aflat.ctypes.data, kp, K, rows,
                                              _KIND_OF[self.dtype], C.byref(self._h)))
        self.state_dim = int(sum(orders))
        self.why_not = lib().wfk_chain_iir_unfused_reason(self._h).decode()

    @property
    def fused(self) -> bool:
        return bool(lib().wfk_chain_iir_is_fused(self._h))

    def launch(self, out_ptr: int, out_stride: int, zi_ptr=None, zf_ptr=None, initial=0.0, stream: int = 0) -> bool:
        """-> False when the library refused the launch with WFK_ETIMEOUT (an earlier launch of this plan ran into a
        look-back timeout; the plan has switched to the unfused three-launch form: launch again)"""
        return _accepted(lib().wfk_chain_iir_launch(self._h, out_ptr, out_stride, zi_ptr, zf_ptr, float(initial),
                                                    stream))

    def status(self, stream=0) -> bool:
        """Synchronise `stream`; False if a launch since the last check timed out in a look-back (outputs hold NaN)"""
        return _accepted(lib().wfk_chain_iir_status(self._h, stream))

    def kernel_name(self) -> str:
        return lib().wfk_chain_iir_kernel_name(self._h).decode()

    def table_bytes(self) -> int:
        return int(lib().wfk_chain_iir_table_bytes(self._h))


class IirPlan(_Handle):
    """Cascade of direct-form-II-transposed sections along each of `batch` rows.

    sections: list of (b, a) coefficient sequences; a section's order is
    max(len(b), len(a)) - 1 (scipy.signal.lfilter convention).  An SOS matrix is the
    list [(row[:3], row[3:]) for row in sos] (scipy.signal.sosfilt)."""
    _destroy = 'wfk_iir_plan_destroy'

    def __init__(self, sections, n: int, batch: int = 1, dtype=np.float64):
        orders, bflat, aflat = _pack_sections(sections)
        self.n, self.batch, self.dtype = int(n), int(batch), np.dtype(dtype)
        check(lib().wfk_iir_plan_create(len(orders), orders.ctypes.data, bflat.ctypes.data,
                                        aflat.ctypes.data, self.n, self.batch,
                                        _KIND_OF[self.dtype], C.byref(self._h)))
        self.state_dim = int(sum(orders))

    def apply(self, in_ptr, in_stride, out_ptr, out_stride, zi_ptr=None, zf_ptr=None,
              initial=0.0, stream=0):
        """-> False when the library refused the launch with WFK_ETIMEOUT: an EARLIER launch of this plan
        (for instance the other row of a complex waveform) ran into a look-back timeout; nothing was
        launched, the plan has switched to the three-launch form -- treat it like `status() == False`."""
        return _accepted(lib().wfk_iir_apply(self._h, in_ptr, in_stride, out_ptr, out_stride, zi_ptr,
                                             zf_ptr, float(initial), stream))

    def status(self, stream=0) -> bool:
        """Synchronise `stream`; False if a single-pass launch since the last check ran into a look-back
        timeout (its outputs hold NaN; the plan has switched to the three-launch form: apply again)."""
        return _accepted(lib().wfk_iir_status(self._h, stream))

    def kernel_name(self) -> str:
        """what the next apply launches, one entry per pass of a cut cascade joined with ' + ':
        'iir_onepass<T,NSEC,ORD,PLAIN>' (+ ' persistent'), 'iir_pass<T,NSEC,ORD>' (three launches), 'iir_scale<T>'"""
        return lib().wfk_iir_kernel_name(self._h).decode()


def pack_sections_rows(sections_per_row):
    """list (one entry per row) of cascades [(b, a), ...] -> (orders int32, b (batch, NC), a (batch, NC), own):
    every section padded with zero coefficients to the widest order of ANY section of any row, and every row to the
    largest section count with pass-through sections (b = [1, 0, ...], a = [1, 0, ...]) -- both exact for the
    direct form II transposed.  `own[r]` lists the orders row r came with (what its zi / zf hold).
    ValueError: no rows, an empty cascade; NotImplementedError: complex coefficients."""
    rows = []
    for secs in sections_per_row:
        row = []
        for b, a in secs:
            b, a = np.atleast_1d(np.asarray(b)), np.atleast_1d(np.asarray(a))
            if np.iscomplexobj(b) or np.iscomplexobj(a):
                raise NotImplementedError('IIR sections with complex coefficients')
            if b.ndim != 1 or a.ndim != 1 or len(a) < 1 or len(b) < 1:
                raise ValueError('a section is a pair of 1-D coefficient sequences (b, a)')
            row.append((b.astype(np.float64), a.astype(np.float64)))
        if not row:
            raise ValueError('a row without sections')
        rows.append(row)
    if not rows:
        raise ValueError('no rows')
    nsec = max(len(r) for r in rows)
    order = max(1, max(max(len(b), len(a)) - 1 for r in rows for b, a in r))
    bm = np.zeros((len(rows), nsec, order + 1))
    am = np.zeros((len(rows), nsec, order + 1))
    bm[:, :, 0] = 1.0
    am[:, :, 0] = 1.0
    own = []
    for r, row in enumerate(rows):
        for s, (b, a) in enumerate(row):
            bm[r, s, :] = 0.0
            am[r, s, :] = 0.0
            bm[r, s, :len(b)] = b
            am[r, s, :len(a)] = a
        own.append([max(len(b), len(a)) - 1 for b, a in row])
    orders = np.full(nsec, order, dtype=np.int32)
    return orders, bm.reshape(len(rows), -1), am.reshape(len(rows), -1), own


class IirRowsPlan(_Handle):
    """One cascade PER ROW (wfk_iir_rows_plan_create): `sections_per_row[r]` is the list of (b, a) sections of
    row r, in IirPlan's conventions.  Rows are padded to a common shape (`pack_sections_rows`); the library takes
    sections of equal order with a total state dimension <= 4 and raises EngineError beyond that.
    `state_dim` is the padded state dimension: zi / zf are (batch, state_dim) device arrays."""
    _destroy = 'wfk_iir_rows_plan_destroy'

    def __init__(self, sections_per_row, n: int, dtype=np.float64):
        orders, bm, am, self.own_orders = pack_sections_rows(sections_per_row)
        self.n, self.batch, self.dtype = int(n), int(bm.shape[0]), np.dtype(dtype)
        self.orders = orders
        bm, am = np.ascontiguousarray(bm), np.ascontiguousarray(am)
        check(lib().wfk_iir_rows_plan_create(len(orders), orders.ctypes.data, bm.ctypes.data, am.ctypes.data,
                                             self.n, self.batch, _KIND_OF[self.dtype], C.byref(self._h)))
        self.state_dim = int(orders.sum())

    def apply(self, in_ptr, in_stride, out_ptr, out_stride, zi_ptr=None, zf_ptr=None, initial_ptr=None, stream=0):
        """initial_ptr: device array of `batch` doubles (one level per row) or None"""
        check(lib().wfk_iir_rows_apply(self._h, in_ptr, in_stride, out_ptr, out_stride, zi_ptr, zf_ptr,
                                       initial_ptr, stream))

    def apply_shared_in(self, in_ptr, out_ptr, out_stride, zi_ptr=None, zf_ptr=None, initial_ptr=None, stream=0):
        """every row reads the SAME n input samples at `in_ptr`; `out` must not overlap them (EngineError)"""
        check(lib().wfk_iir_rows_apply_shared_in(self._h, in_ptr, out_ptr, out_stride, zi_ptr, zf_ptr,
                                                 initial_ptr, stream))

    def kernel_name(self) -> str:
        return lib().wfk_iir_rows_kernel_name(self._h).decode()


class ChainIirRowsPlan(_Handle):
    """sampler -> per-row IIR for every channel of `prog` on `grid` (wfk_chain_iir_rows_*), the twin of ChainIirPlan
    with one cascade PER CHANNEL: `sections_per_row[c]` is the list of (b, a) sections of channel c, packed by
    `pack_sections_rows` (IirRowsPlan's shapes and limits).  Fused, the workgroup that owns a row evaluates each tile
    of the row in LDS and filters it there ('iir_rows_sampled<...>' on fine grids, 'iir_rows_short<...>' at AWG
    rates): the unfiltered samples never touch HBM (`fused`, `why_not`, `kernel_name()`)."""
    _destroy = 'wfk_chain_iir_rows_plan_destroy'

    def __init__(self, prog: Program, grid: wfk_grid, sections_per_row, dtype=np.float64, packed=None):
        """packed: what pack_sections_rows(sections_per_row) gave a caller that has packed the cascades already"""
        orders, bm, am, self.own_orders = pack_sections_rows(sections_per_row) if packed is None else packed
        if bm.shape[0] != prog.n_channels:
            raise ValueError(f'{bm.shape[0]} cascades for {prog.n_channels} rows')
        self.prog, self.grid, self.dtype = prog, grid, np.dtype(dtype)
        self.n, self.n_channels = int(grid.n), prog.n_channels
        self.orders = orders
        bm, am = np.ascontiguousarray(bm), np.ascontiguousarray(am)
        check(lib().wfk_chain_iir_rows_plan_create(C.byref(prog.struct), C.byref(grid), len(orders), orders.ctypes.data,
                                                   bm.ctypes.data, am.ctypes.data, _KIND_OF[self.dtype],
                                                   C.byref(self._h)))
        self.state_dim = int(orders.sum())
        self.fused = bool(lib().wfk_chain_iir_rows_is_fused(self._h))
        self.why_not = lib().wfk_chain_iir_rows_unfused_reason(self._h).decode()

    def launch(self, out_ptr: int, out_stride: int, zi_ptr=None, zf_ptr=None, initial_ptr=None, stream: int = 0):
        """initial_ptr: device array of `n_channels` doubles (one level per row) or None"""
        check(lib().wfk_chain_iir_rows_launch(self._h, out_ptr, out_stride, zi_ptr, zf_ptr, initial_ptr, stream))

    def kernel_name(self) -> str:
        """'iir_rows_sampled<T,NSEC,ORD>', 'iir_rows_short<T,NSEC,ORD>', or the unfused pair joined with ' + '"""
        return lib().wfk_chain_iir_rows_kernel_name(self._h).decode()

    def table_bytes(self) -> int:
        return int(lib().wfk_chain_iir_rows_table_bytes(self._h))


class SpectralPlan(_Handle):
    """out = irfft(rfft(x) * H) along each of `batch` contiguous rows of n samples."""
    _destroy = 'wfk_spectral_plan_destroy'

    def __init__(self, n: int, batch: int = 1, dtype=np.float64):
        self.n, self.batch, self.dtype = int(n), int(batch), np.dtype(dtype)
        check(lib().wfk_spectral_plan_create(self.n, self.batch, _KIND_OF[self.dtype],
                                             C.byref(self._h)))

    def apply(self, in_ptr, out_ptr, H_ptr, stream=0):
        check(lib().wfk_spectral_apply(self._h, in_ptr, out_ptr, H_ptr, stream))


SPEC_ROWS_MAX_TERMS = 8                                    # WFK_SPEC_ROWS_MAX_TERMS of include/wfk.h
SPEC_KINDS = {'reflect': 0, 'correct': 1, 'delay': 2}      # WFK_SPEC_REFLECT / CORRECT / DELAY
SPEC_TERM = np.dtype([('kind', np.int32), ('reserved', np.int32), ('A', np.float64), ('tau', np.float64)])


def pack_spec_terms(terms_rows):
    """list (one entry per row) of term lists -> (terms, counts): the wfk_spec_term records of all rows back to back
    and the int32 number of terms per row.  A term is ('reflect', A, tau), ('correct', A, tau) or ('delay', tau).
    ValueError: no rows, an unknown kind, a term of the wrong length, more than SPEC_ROWS_MAX_TERMS terms in a row,
    a tau that is not finite, |A| >= 1 (A = 1 divides by zero in the reference's filter)."""
    rows = [list(r) for r in terms_rows]
    if not rows:
        raise ValueError('no rows')
    recs = []
    for r, row in enumerate(rows):
        if len(row) > SPEC_ROWS_MAX_TERMS:
            raise ValueError(f'row {r}: {len(row)} terms, a row takes at most {SPEC_ROWS_MAX_TERMS}')
        for term in row:
            term = tuple(term)
            kind = term[0] if term else None
            if not isinstance(kind, str) or kind not in SPEC_KINDS:
                raise ValueError(f"row {r}: a term is ('reflect' | 'correct', A, tau) or ('delay', tau), got {term!r}")
            if len(term) != (2 if kind == 'delay' else 3):
                raise ValueError(f"row {r}: a term is ('reflect' | 'correct', A, tau) or ('delay', tau), got {term!r}")
            A, tau = (0.0, float(term[1])) if kind == 'delay' else (float(term[1]), float(term[2]))
            if not np.isfinite(tau):
                raise ValueError(f'row {r}: tau is not finite')
            if not abs(A) < 1.0:
                raise ValueError(f'row {r}: a reflection needs |A| < 1, got {A!r}')
            recs.append((SPEC_KINDS[kind], 0, A, tau))
    return (np.array(recs, dtype=SPEC_TERM).reshape(-1),
            np.array([len(row) for row in rows], dtype=np.int32))


def spec_phase_step(tau: float, sample_rate: float, n: int):
    """(hi, lo): tau * sample_rate / n as the pair of doubles a SpectralRowsPlan stores (host only, no device)"""
    hi, lo = C.c_double(), C.c_double()
    check(lib().wfk_spectral_rows_phase_step(float(tau), float(sample_rate), int(n), C.byref(hi), C.byref(lo)))
    return hi.value, lo.value


def _real_dtype(dtype, complex_is_pending=True):
    """the np.dtype of a plan's rows is float64 or float32: ValueError otherwise, but NotImplementedError for a complex
    one where `complex_is_pending`"""
    if dtype.kind == 'c' and complex_is_pending:
        raise NotImplementedError('complex rows')
    if dtype not in (np.dtype(np.float64), np.dtype(np.float32)):
        raise ValueError('dtype must be float64 or float32')


class SpectralRowsPlan(_Handle):
    """out[r] = irfft(rfft(x[r]) * H_r): every row its own product of reflection / inverse-reflection / delay terms
    (`pack_spec_terms`), H formed on the device (wfk_spectral_rows_plan_create).  `batch` = len(terms_rows)."""
    _destroy = 'wfk_spectral_rows_plan_destroy'

    def __init__(self, terms_rows, n: int, sample_rate: float, dtype=np.float64):
        terms, counts = pack_spec_terms(terms_rows)
        self.n, self.batch, self.dtype = int(n), len(counts), np.dtype(dtype)
        self.sample_rate = float(sample_rate)
        _real_dtype(self.dtype, complex_is_pending=False)
        if self.n < 1 or not (np.isfinite(self.sample_rate) and self.sample_rate > 0):
            raise ValueError('n >= 1 and a positive sample_rate')
        check(lib().wfk_spectral_rows_plan_create(self.n, self.batch, _KIND_OF[self.dtype], self.sample_rate,
                                                  terms.ctypes.data if len(terms) else None, counts.ctypes.data,
                                                  C.byref(self._h)))

    def apply(self, in_ptr, in_stride, out_ptr, out_stride, stream=0):
        check(lib().wfk_spectral_rows_apply(self._h, in_ptr, in_stride, out_ptr, out_stride, stream))


class ShiftRowsPlan(_Handle):
    """out[r] = the reference's shift of x[r] by points[r] whole samples and the fraction deltas[r] of one (linear
    interpolation, zero fill; wfk_shift_rows_plan_create).  `batch` = len(points).  ValueError before any device
    work: no rows, lengths that differ, n < 0, a delta outside [0, 1] or not finite, a dtype other than float64 /
    float32 (NotImplementedError for a complex one).  |points| is clamped to 2**62: such a row is all zero either way."""
    _destroy = 'wfk_shift_rows_plan_destroy'

    def __init__(self, points, deltas, n: int, dtype=np.float64):
        self.n, self.dtype = int(n), np.dtype(dtype)
        _real_dtype(self.dtype)
        pts = [max(-2**62, min(2**62, int(p))) for p in np.asarray(points, dtype=object).reshape(-1)]
        self.points = np.array(pts, dtype=np.int64)
        self.deltas = np.ascontiguousarray(deltas, dtype=np.float64).reshape(-1)
        self.batch = len(self.points)
        if self.batch < 1 or len(self.deltas) != self.batch:
            raise ValueError(f'{self.batch} points and {len(self.deltas)} deltas: one of each per row, at least one row')
        if self.n < 0:
            raise ValueError('n >= 0')
        if not np.all((self.deltas >= 0.0) & (self.deltas <= 1.0)):
            raise ValueError('every delta must lie in [0, 1]')
        check(lib().wfk_shift_rows_plan_create(self.n, self.batch, _KIND_OF[self.dtype], self.points.ctypes.data,
                                               self.deltas.ctypes.data, C.byref(self._h)))

    def apply(self, in_ptr, in_stride, out_ptr, out_stride, stream=0):
        check(lib().wfk_shift_rows_apply(self._h, in_ptr, in_stride, out_ptr, out_stride, stream))

    def kernel_name(self) -> str:
        return lib().wfk_shift_rows_kernel_name(self._h).decode()


def dac_rows_arguments(gain, offset, n, bits=16, shift=0, interleave=1, dtype=np.float64):
    """the arguments of a DacRowsPlan, checked on the host -> (gain, offset: float64 arrays of one length, n, bits,
    shift, interleave, dtype).  ValueError / NotImplementedError as DacRowsPlan lists them."""
    n, bits, shift, interleave, dtype = int(n), int(bits), int(shift), int(interleave), np.dtype(dtype)
    _real_dtype(dtype)
    gain = np.ascontiguousarray(gain, dtype=np.float64).reshape(-1)
    offset = np.ascontiguousarray(offset, dtype=np.float64).reshape(-1)
    if len(gain) < 1 or len(offset) != len(gain):
        raise ValueError(f'{len(gain)} gains and {len(offset)} offsets: one of each per row, at least one row')
    if n < 0:
        raise ValueError('n >= 0')
    if not 2 <= bits <= 16:
        raise ValueError('bits must lie in [2, 16]')
    if not 0 <= shift <= 16 - bits:
        raise ValueError(f'shift must lie in [0, 16 - bits] = [0, {16 - bits}]')
    if interleave not in (1, 2):
        raise ValueError('interleave must be 1 or 2')
    if len(gain) % interleave:
        raise ValueError(f'{len(gain)} rows are no multiple of the interleave {interleave}')
    for name, a in (('gain', gain), ('offset', offset)):
        bad = np.flatnonzero(~np.isfinite(a))
        if len(bad):
            raise ValueError(f'row {int(bad[0])}: {name} is not finite')
    return gain, offset, n, bits, shift, interleave, dtype


class DacRowsPlan(_Handle):
    """codes[r] = saturate(rint(x[r] * gain[r] + offset[r])) * 2**shift as int16 for `batch` = len(gain) rows of n
    float64 / float32 samples (the product and the sum each rounded, half to even, clamped to `bits` signed bits; NaN
    gives 0), `interleave` input rows sample-interleaved into one output row (wfk_dac_rows_plan_create).
    `.lo` / `.hi`: the rails; `.out_rows`, `.out_n`: the shape of the result.  ValueError before any device work:
    no rows, lengths that differ, n < 0, bits outside [2, 16], shift outside [0, 16 - bits], an interleave other
    than 1 or 2, a batch that is no multiple of it, a gain or offset that is not finite, a dtype other than float64 /
    float32 (NotImplementedError for a complex one)."""
    _destroy = 'wfk_dac_rows_plan_destroy'

    def __init__(self, gain, offset, n: int, bits: int = 16, shift: int = 0, interleave: int = 1, dtype=np.float64):
        (self.gain, self.offset, self.n, self.bits, self.shift, self.interleave,
         self.dtype) = dac_rows_arguments(gain, offset, n, bits, shift, interleave, dtype)
        self.batch = len(self.gain)
        self.lo, self.hi = -2**(self.bits - 1), 2**(self.bits - 1) - 1
        self.out_rows, self.out_n = self.batch // self.interleave, self.interleave * self.n
        check(lib().wfk_dac_rows_plan_create(self.n, self.batch, _KIND_OF[self.dtype], self.gain.ctypes.data,
                                             self.offset.ctypes.data, self.bits, self.shift, self.interleave,
                                             C.byref(self._h)))

    def apply(self, in_ptr, in_stride, out_ptr, out_stride, counts_ptr=None, stream=0):
        """counts_ptr: None, or batch * 3 int64 on the device, overwritten with [below, above, nan] per input row"""
        check(lib().wfk_dac_rows_apply(self._h, in_ptr, in_stride, out_ptr, out_stride, counts_ptr, stream))

    def kernel_name(self, counts: bool = False) -> str:
        return lib().wfk_dac_rows_kernel_name(self._h, 1 if counts else 0).decode()


class IirRowsDacPlan(_Handle):
    """IirRowsPlan(sections_per_row, n, dtype) followed by DacRowsPlan(gain, offset, n, bits, shift, 1, dtype), bit for
    bit -- codes, counts and final states -- in one kernel, 'iir_rows_dac<T,NSEC,ORD>', without the float rows between
    the two (wfk_iir_rows_dac_plan_create).  One cascade and one gain and offset per row; the errors of both parents,
    the converter's first, before any device work.  `state_dim`, `own_orders`, `orders` as IirRowsPlan; `.lo` / `.hi`:
    the rails."""
    _destroy = 'wfk_iir_rows_dac_plan_destroy'

    def __init__(self, sections_per_row, gain, offset, n: int, bits: int = 16, shift: int = 0, dtype=np.float64,
                 packed=None):
        (self.gain, self.offset, self.n, self.bits, self.shift, _,
         self.dtype) = dac_rows_arguments(gain, offset, n, bits, shift, 1, dtype)
        orders, bm, am, self.own_orders = packed if packed is not None else pack_sections_rows(sections_per_row)
        self.batch, self.orders = int(bm.shape[0]), orders
        if len(self.gain) != self.batch:
            raise ValueError(f'{len(self.gain)} gains for {self.batch} rows')
        self.lo, self.hi = -2**(self.bits - 1), 2**(self.bits - 1) - 1
        bm, am = np.ascontiguousarray(bm), np.ascontiguousarray(am)
        check(lib().wfk_iir_rows_dac_plan_create(len(orders), orders.ctypes.data, bm.ctypes.data, am.ctypes.data,
                                                 self.n, self.batch, _KIND_OF[self.dtype], self.gain.ctypes.data,
                                                 self.offset.ctypes.data, self.bits, self.shift, C.byref(self._h)))
        self.state_dim = int(orders.sum())

    def apply(self, in_ptr, in_stride, out_ptr, out_stride, counts_ptr=None, zi_ptr=None, zf_ptr=None,
              initial_ptr=None, stream=0):
        """counts_ptr: None, or batch * 3 int64 on the device, overwritten with [below, above, nan] per row;
        initial_ptr: device array of `batch` doubles (one level per row) or None"""
        check(lib().wfk_iir_rows_dac_apply(self._h, in_ptr, in_stride, out_ptr, out_stride, counts_ptr, zi_ptr, zf_ptr,
                                           initial_ptr, stream))

    def apply_shared_in(self, in_ptr, out_ptr, out_stride, counts_ptr=None, zi_ptr=None, zf_ptr=None,
                        initial_ptr=None, stream=0):
        """every row reads the SAME n input samples at `in_ptr`"""
        check(lib().wfk_iir_rows_dac_apply_shared_in(self._h, in_ptr, out_ptr, out_stride, counts_ptr, zi_ptr, zf_ptr,
                                                     initial_ptr, stream))

    def kernel_name(self) -> str:
        return lib().wfk_iir_rows_dac_kernel_name(self._h).decode()


class ChainIirRowsDacPlan(_Handle):
    """sampler -> per-row IIR -> DAC codes for every channel of `prog` on `grid` (wfk_chain_iir_rows_dac_*):
    ChainIirRowsPlan (float64) followed by DacRowsPlan, bit for bit.  Where ChainIirRowsPlan fuses, the same fill runs
    in front of the codes store ('iir_rows_sampled_dac<f64,NSEC,ORD>' on fine grids, 'iir_rows_short_dac<...>' at AWG
    rates: 2 B per sample of HBM traffic); everything else (`why_not`) runs the sampler into a float64 scratch the
    caller lends, then 'iir_rows_dac<f64,NSEC,ORD>'."""
    _destroy = 'wfk_chain_iir_rows_dac_plan_destroy'

    def __init__(self, prog: Program, grid: wfk_grid, sections_per_row, gain, offset, bits: int = 16, shift: int = 0,
                 packed=None):
        (self.gain, self.offset, self.n, self.bits, self.shift, _,
         _) = dac_rows_arguments(gain, offset, int(grid.n), bits, shift, 1)
        orders, bm, am, self.own_orders = pack_sections_rows(sections_per_row) if packed is None else packed
        if bm.shape[0] != prog.n_channels:
            raise ValueError(f'{bm.shape[0]} cascades for {prog.n_channels} rows')
        if len(self.gain) != prog.n_channels:
            raise ValueError(f'{len(self.gain)} gains for {prog.n_channels} rows')
        self.prog, self.grid, self.n_channels, self.orders = prog, grid, prog.n_channels, orders
        self.lo, self.hi = -2**(self.bits - 1), 2**(self.bits - 1) - 1
        bm, am = np.ascontiguousarray(bm), np.ascontiguousarray(am)
        check(lib().wfk_chain_iir_rows_dac_plan_create(C.byref(prog.struct), C.byref(grid), len(orders),
                                                       orders.ctypes.data, bm.ctypes.data, am.ctypes.data,
                                                       self.gain.ctypes.data, self.offset.ctypes.data, self.bits,
                                                       self.shift, C.byref(self._h)))
        self.state_dim = int(orders.sum())
        self.fused = bool(lib().wfk_chain_iir_rows_dac_is_fused(self._h))
        self.why_not = lib().wfk_chain_iir_rows_dac_unfused_reason(self._h).decode()

    def launch(self, out_ptr, out_stride, counts_ptr=None, scratch_ptr=None, scratch_stride=0, zi_ptr=None, zf_ptr=None,
               initial_ptr=None, stream=0):
        """counts_ptr: None, or n_channels * 3 int64 on the device, overwritten; scratch_ptr: n_channels float64 rows
        `scratch_stride` apart, which an unfused plan needs and a fused one does not touch"""
        check(lib().wfk_chain_iir_rows_dac_launch(self._h, out_ptr, out_stride, counts_ptr, scratch_ptr, scratch_stride,
                                                  zi_ptr, zf_ptr, initial_ptr, stream))

    def kernel_name(self) -> str:
        """'iir_rows_sampled_dac<f64,NSEC,ORD>', 'iir_rows_short_dac<f64,NSEC,ORD>', or the sampler's kernels and
        'iir_rows_dac<f64,NSEC,ORD>' joined with ' + '"""
        return lib().wfk_chain_iir_rows_dac_kernel_name(self._h).decode()

    def table_bytes(self) -> int:
        return int(lib().wfk_chain_iir_rows_dac_table_bytes(self._h))


class ChainDacPlan(_Handle):
    """sampler -> DAC codes for every channel of `prog` on `grid` (wfk_chain_dac_*): DacRowsPlan's arithmetic and
    arguments (one gain and offset per channel, float64 samples) on what Plan(prog, grid) samples.  Fused -- a pure
    short-tier plan, interleave 1 -- the sampler's own kernel stores the int16 codes
    ('wfk_sample_short_dac<16,FAM,COUNT>') and the float64 rows never exist; everything else (`why_not`) runs the
    sampler into a float64 scratch the caller lends, then dac_rows.  Codes and counts are those of the two launches
    bit for bit either way."""
    _destroy = 'wfk_chain_dac_plan_destroy'

    def __init__(self, prog: Program, grid: wfk_grid, gain, offset, bits: int = 16, shift: int = 0, interleave: int = 1):
        (self.gain, self.offset, self.n, self.bits, self.shift, self.interleave,
         _) = dac_rows_arguments(gain, offset, int(grid.n), bits, shift, interleave)
        if len(self.gain) != prog.n_channels:
            raise ValueError(f'{len(self.gain)} gains for {prog.n_channels} rows')
        self.prog, self.grid, self.n_channels = prog, grid, prog.n_channels
        self.lo, self.hi = -2**(self.bits - 1), 2**(self.bits - 1) - 1
        self.out_rows, self.out_n = self.n_channels // self.interleave, self.interleave * self.n
        check(lib().wfk_chain_dac_plan_create(C.byref(prog.struct), C.byref(grid), self.gain.ctypes.data,
                                              self.offset.ctypes.data, self.bits, self.shift, self.interleave,
                                              C.byref(self._h)))
        self.fused = bool(lib().wfk_chain_dac_is_fused(self._h))
        self.why_not = lib().wfk_chain_dac_unfused_reason(self._h).decode()

    def launch(self, out_ptr, out_stride, counts_ptr=None, scratch_ptr=None, scratch_stride=0, stream=0):
        """counts_ptr: None, or n_channels * 3 int64 on the device, overwritten; scratch_ptr: n_channels float64 rows
        `scratch_stride` apart, which an unfused plan needs and a fused one does not touch"""
        check(lib().wfk_chain_dac_launch(self._h, out_ptr, out_stride, counts_ptr, scratch_ptr, scratch_stride, stream))

    def kernel_name(self, counts: bool = False) -> str:
        """'wfk_sample_short_dac<16,FAM,COUNT>', or the sampler's kernels and dac_rows' joined with ' + '"""
        return lib().wfk_chain_dac_kernel_name(self._h, 1 if counts else 0).decode()

    def table_bytes(self) -> int:
        return int(lib().wfk_chain_dac_table_bytes(self._h))


MARKER_MAX_EDGE = 4096     # WFK_MARKER_MAX_EDGE


def marker_rows_arguments(threshold, lead, trail, n, group=1, dtype=np.float64):
    """the arguments of a MarkerRowsPlan, checked on the host -> (threshold: float64, lead, trail: int32 arrays of one
    length, one entry per MARKER row, n, group, dtype).  ValueError / NotImplementedError as MarkerRowsPlan lists them."""
    n, group, dtype = int(n), int(group), np.dtype(dtype)
    _real_dtype(dtype)
    threshold = np.ascontiguousarray(threshold, dtype=np.float64).reshape(-1)
    edges = []
    for name, v in (('lead', lead), ('trail', trail)):
        a = np.asarray(v).reshape(-1)
        if a.dtype.kind not in 'iu' and not (a.dtype.kind == 'f' and np.all(np.isfinite(a)) and np.all(a == np.rint(a))):
            raise ValueError(f'{name} is a number of samples: integers, got {a.dtype}')
        edges.append(np.array([int(e) for e in a], dtype=object))
    if len(threshold) < 1 or len(edges[0]) != len(threshold) or len(edges[1]) != len(threshold):
        raise ValueError(f'{len(threshold)} thresholds, {len(edges[0])} leads and {len(edges[1])} trails: one of each '
                         f'per marker row, at least one row')
    if n < 0:
        raise ValueError('n >= 0')
    if group not in (1, 2):
        raise ValueError('group must be 1 or 2')
    bad = np.flatnonzero(~np.isfinite(threshold))
    if len(bad):
        raise ValueError(f'row {int(bad[0])}: threshold is not finite')
    bad = np.flatnonzero(threshold < 0.0)
    if len(bad):
        raise ValueError(f'row {int(bad[0])}: threshold is negative')
    for name, a in zip(('lead', 'trail'), edges):
        for r, e in enumerate(a):
            if e < 0:
                raise ValueError(f'row {r}: {name} is negative')
            if e > MARKER_MAX_EDGE:
                raise ValueError(f'row {r}: {name} exceeds {MARKER_MAX_EDGE}')
    return threshold, edges[0].astype(np.int32), edges[1].astype(np.int32), n, group, dtype


class MarkerRowsPlan(_Handle):
    """m[g, i] = any |x[g k + j, i']| > threshold[g] over the k = `group` input rows of marker row g and i' in
    [i - trail[g], i + lead[g]] (clipped to the row), for `batch` = group * len(threshold) rows of n float64 / float32
    samples: as uint8 0 / 1 (`apply`), or written into bit `bit` of int16 codes in the layout
    DacRowsPlan(interleave=group) produces (`apply_codes`) (wfk_marker_rows_plan_create).  `.out_rows`: the marker
    rows.  ValueError before any device work: no rows, lengths that differ, n < 0, a group other than 1 or 2, a
    threshold that is negative or not finite, a lead or trail that is no integer, negative or above MARKER_MAX_EDGE
    (the row is named), a dtype other than float64 / float32 (NotImplementedError for a complex one)."""
    _destroy = 'wfk_marker_rows_plan_destroy'

    def __init__(self, threshold, lead, trail, n: int, group: int = 1, dtype=np.float64):
        (self.threshold, self.lead, self.trail, self.n, self.group,
         self.dtype) = marker_rows_arguments(threshold, lead, trail, n, group, dtype)
        self.out_rows = len(self.threshold)
        self.batch = self.out_rows * self.group
        check(lib().wfk_marker_rows_plan_create(self.n, self.batch, _KIND_OF[self.dtype], self.group,
                                                self.threshold.ctypes.data, self.lead.ctypes.data,
                                                self.trail.ctypes.data, C.byref(self._h)))

    def apply(self, in_ptr, in_stride, out_ptr, out_stride, counts_ptr=None, stream=0):
        """counts_ptr: None, or out_rows * 2 int64 on the device, overwritten with [high, pulses] per marker row"""
        check(lib().wfk_marker_rows_apply(self._h, in_ptr, in_stride, out_ptr, out_stride, counts_ptr, stream))

    def apply_codes(self, in_ptr, in_stride, codes_ptr, codes_stride, bit=0, counts_ptr=None, stream=0):
        if not 0 <= int(bit) <= 15:
            raise ValueError('bit must lie in [0, 15]')
        check(lib().wfk_marker_rows_apply_codes(self._h, in_ptr, in_stride, codes_ptr, codes_stride, int(bit),
                                                counts_ptr, stream))

    def span(self, codes: bool = False) -> int:
        """the samples one workgroup covers in that form"""
        return int(lib().wfk_marker_rows_span(self._h, 1 if codes else 0))

    def kernel_name(self, codes: bool = False, counts: bool = False) -> str:
        return lib().wfk_marker_rows_kernel_name(self._h, 1 if codes else 0, 1 if counts else 0).decode()


SEGMENT_MAX_ALIGN = 4096   # WFK_SEGMENT_MAX_ALIGN


def _whole(name, v):
    """v as an int; ValueError where it is no whole number"""
    a = np.asarray(v)
    if a.ndim != 0 or a.dtype.kind == 'b' or not (a.dtype.kind in 'iu' or (a.dtype.kind == 'f' and np.isfinite(a)
                                                                          and a == np.rint(a))):
        raise ValueError(f'{name} must be a whole number')
    return int(a)


def segment_rows_arguments(n, rows=1, width=1, align=1, max_segments=None, capacity=None):
    """the arguments of a SegmentRowsPlan, checked on the host (no device, no library) -> (n, rows, width, align,
    max_segments, capacity) as ints.  `max_segments` None: ceil(ceil(n / align) / 2), the most segments a row can
    have; `capacity` None: n.  ValueError, the argument named: n outside [0, 2^31 - 1], rows < 1, a width other than 1
    or 2, an align that is no power of two in [1, SEGMENT_MAX_ALIGN], max_segments < 0, capacity outside [0, n]."""
    n, rows, width, align = _whole('n', n), _whole('rows', rows), _whole('width', width), _whole('align', align)
    if not 0 <= n <= 2**31 - 1:
        raise ValueError('n must lie in [0, 2^31 - 1]')
    if rows < 1:
        raise ValueError('rows must be at least 1')
    if width not in (1, 2):
        raise ValueError('width must be 1 or 2')
    if not 1 <= align <= SEGMENT_MAX_ALIGN or align & (align - 1):
        raise ValueError(f'align must be a power of two in [1, {SEGMENT_MAX_ALIGN}]')
    granules = -(-n // align)
    max_segments = (granules + 1) // 2 if max_segments is None else _whole('max_segments', max_segments)
    capacity = n if capacity is None else _whole('capacity', capacity)
    if max_segments < 0:
        raise ValueError('max_segments must not be negative')
    if not 0 <= capacity <= n:
        raise ValueError('capacity must lie in [0, n]')
    return n, rows, width, align, max_segments, capacity


class SegmentRowsPlan(_Handle):
    """`rows` rows of `width` * n int16 codes cut at their marker in granules of `align` samples: a table of
    [start, length, offset] per segment, the kept codes packed back to back and [count, kept] per row
    (wfk_segment_rows_plan_create; the semantics are in include/wfk.h).  The plan owns the workspace its three launches
    share: one stream at a time.  ValueError before any device work as `segment_rows_arguments` lists them."""
    _destroy = 'wfk_segment_rows_plan_destroy'

    def __init__(self, n, rows=1, width=1, align=1, max_segments=None, capacity=None):
        (self.n, self.rows, self.width, self.align, self.max_segments,
         self.capacity) = segment_rows_arguments(n, rows, width, align, max_segments, capacity)
        check(lib().wfk_segment_rows_plan_create(self.n, self.rows, self.width, self.align, self.max_segments,
                                                 self.capacity, C.byref(self._h)))

    def apply_bit(self, codes_ptr, codes_stride, bit, table_ptr, table_stride, packed_ptr, packed_stride, used_ptr,
                  stream=0):
        """table_ptr = packed_ptr = None: the sizing pass; used_ptr: rows * 2 int64, overwritten with [count, kept]"""
        if not 0 <= int(bit) <= 15:
            raise ValueError('bit must lie in [0, 15]')
        check(lib().wfk_segment_rows_apply_bit(self._h, codes_ptr, codes_stride, int(bit), table_ptr, table_stride,
                                               packed_ptr, packed_stride, used_ptr, stream))

    def apply_marks(self, codes_ptr, codes_stride, marks_ptr, marks_stride, table_ptr, table_stride, packed_ptr,
                    packed_stride, used_ptr, stream=0):
        check(lib().wfk_segment_rows_apply_marks(self._h, codes_ptr, codes_stride, marks_ptr, marks_stride, table_ptr,
                                                 table_stride, packed_ptr, packed_stride, used_ptr, stream))

    def span(self) -> int:
        """the samples one workgroup covers"""
        return int(lib().wfk_segment_rows_span(self._h))

    def kernel_name(self, launch: int = 0, marks: bool = False) -> str:
        """launch 0, 1, 2: the count, scan and pack kernels"""
        return lib().wfk_segment_rows_kernel_name(self._h, int(launch), 1 if marks else 0).decode()


def segment_library_arguments(rows=1, width=1, max_segments=0, capacity=0, lib_capacity=None):
    """the arguments of a SegmentLibraryPlan, checked on the host (no device, no library) -> (rows, width,
    max_segments, capacity, lib_capacity) as ints.  `lib_capacity` None: capacity.  ValueError, the argument named:
    rows < 1, a width other than 1 or 2, max_segments outside [0, 2^30], capacity outside [0, 2^31 - 1], lib_capacity
    outside [0, capacity]."""
    rows, width = _whole('rows', rows), _whole('width', width)
    max_segments, capacity = _whole('max_segments', max_segments), _whole('capacity', capacity)
    if rows < 1:
        raise ValueError('rows must be at least 1')
    if width not in (1, 2):
        raise ValueError('width must be 1 or 2')
    if max_segments < 0:
        raise ValueError('max_segments must not be negative')
    if max_segments > 2**30:
        raise ValueError('max_segments must not exceed 2^30')
    if not 0 <= capacity <= 2**31 - 1:
        raise ValueError('capacity must lie in [0, 2^31 - 1]')
    lib_capacity = capacity if lib_capacity is None else _whole('lib_capacity', lib_capacity)
    if not 0 <= lib_capacity <= capacity:
        raise ValueError('lib_capacity must lie in [0, capacity]')
    return rows, width, max_segments, capacity, lib_capacity


class SegmentLibraryPlan(_Handle):
    """The waveform library of `rows` rows that a SegmentRowsPlan of this width, max_segments and capacity cut: equal
    segments of a row share one slot (wfk_segment_library_plan_create; the semantics are in include/wfk.h).  The plan
    owns the workspace its launches share: one stream at a time.  WFK_SEGLIB_HASH_BITS is read here.  ValueError
    before any device work as `segment_library_arguments` lists them."""
    _destroy = 'wfk_segment_library_plan_destroy'

    def __init__(self, rows=1, width=1, max_segments=0, capacity=0, lib_capacity=None):
        (self.rows, self.width, self.max_segments, self.capacity,
         self.lib_capacity) = segment_library_arguments(rows, width, max_segments, capacity, lib_capacity)
        check(lib().wfk_segment_library_plan_create(self.rows, self.width, self.max_segments, self.capacity,
                                                    self.lib_capacity, C.byref(self._h)))

    def apply(self, table_ptr, table_stride, packed_ptr, packed_stride, used_ptr, plays_ptr, plays_stride, slots_ptr,
              slots_stride, library_ptr, library_stride, lib_used_ptr, stream=0):
        """plays_ptr, slots_ptr, library_ptr: each None or an output; all None: the sizing pass; lib_used_ptr: rows * 2
        int64, overwritten with [unique, lib_kept], [-1, -1] for a row that cannot be read"""
        check(lib().wfk_segment_library_apply(self._h, table_ptr, table_stride, packed_ptr, packed_stride, used_ptr,
                                              plays_ptr, plays_stride, slots_ptr, slots_stride, library_ptr,
                                              library_stride, lib_used_ptr, stream))

    def kernel_name(self, launch: int = 0) -> str:
        """launch 0 .. 3: the hash, match, scan and copy kernels"""
        return lib().wfk_segment_library_kernel_name(self._h, int(launch)).decode()


def segment_play_arguments(n, rows=1, width=1, max_segments=0, capacity=0):
    """the arguments of a SegmentPlayPlan, checked on the host (no device, no library) -> (n, rows, width,
    max_segments, capacity) as ints.  ValueError, the argument named: n outside [0, 2^31 - 1], rows < 1, a width other
    than 1 or 2, max_segments outside [0, 2^30], capacity outside [0, 2^31 - 1]."""
    n, rows, width = _whole('n', n), _whole('rows', rows), _whole('width', width)
    max_segments, capacity = _whole('max_segments', max_segments), _whole('capacity', capacity)
    if not 0 <= n <= 2**31 - 1:
        raise ValueError('n must lie in [0, 2^31 - 1]')
    if rows < 1:
        raise ValueError('rows must be at least 1')
    if width not in (1, 2):
        raise ValueError('width must be 1 or 2')
    if max_segments < 0:
        raise ValueError('max_segments must not be negative')
    if max_segments > 2**30:
        raise ValueError('max_segments must not exceed 2^30')
    if not 0 <= capacity <= 2**31 - 1:
        raise ValueError('capacity must lie in [0, 2^31 - 1]')
    return n, rows, width, max_segments, capacity


def segment_play_idle(idle, width):
    """`idle` -- one int16 code, or one per code of a sample -- as the `width` codes an apply is given -> (idle0,
    idle1) as ints (width 1: idle1 = idle0).  ValueError: another number of codes, a code that is no whole number in
    [-32768, 32767]."""
    a = np.asarray(idle).reshape(-1)
    if len(a) not in (1, int(width)):
        raise ValueError('idle is one code or one per code of a sample')
    codes = [_whole('idle', v) for v in a]
    if not all(-32768 <= c <= 32767 for c in codes):
        raise ValueError('idle must lie in [-32768, 32767]')
    return codes[0], codes[-1]


class SegmentPlayPlan(_Handle):
    """`rows` rows of `width` * n int16 codes played back from a segment table and a waveform memory, with the report
    [played, differ, stray, first] per row (wfk_segment_play_plan_create; the semantics are in include/wfk.h).  The plan
    owns the workspace its two launches share: one stream at a time.  ValueError before any device work as
    `segment_play_arguments` lists them."""
    _destroy = 'wfk_segment_play_plan_destroy'

    def __init__(self, n, rows=1, width=1, max_segments=0, capacity=0):
        (self.n, self.rows, self.width, self.max_segments,
         self.capacity) = segment_play_arguments(n, rows, width, max_segments, capacity)
        check(lib().wfk_segment_play_plan_create(self.n, self.rows, self.width, self.max_segments, self.capacity,
                                                 C.byref(self._h)))

    def apply(self, table_ptr, table_stride, packed_ptr, packed_stride, used_ptr, idle, out_ptr, out_stride,
              expect_ptr, expect_stride, report_ptr, stream=0):
        """idle: (idle0, idle1), by value; out_ptr, expect_ptr: each None or a side; both None: the checking pass;
        report_ptr: rows * 4 int64, overwritten with [played, differ, stray, first], all -1 for a bad row"""
        check(lib().wfk_segment_play_apply(self._h, table_ptr, table_stride, packed_ptr, packed_stride, used_ptr,
                                           int(idle[0]), int(idle[1]), out_ptr, out_stride, expect_ptr, expect_stride,
                                           report_ptr, stream))

    def span(self) -> int:
        """the samples one workgroup of the second launch covers"""
        return int(lib().wfk_segment_play_span(self._h))

    def kernel_name(self, launch: int = 0) -> str:
        """launch 0: the check; 1, 2, 3: the fill of a play, of a verifying pass, of both"""
        return lib().wfk_segment_play_kernel_name(self._h, int(launch)).decode()


MIX_TILE_ROWS = 8          # WFK_MIX_TILE_ROWS


def _mix_rows_csr(matrix):
    """-> (rows_out, rows_in, row_ptr, col, val) of a 2-D array-like (its non-zero entries, row by row) or of an object
    with `.tocsr()` (scipy.sparse: indptr / indices / data as they are stored); nothing is checked beyond the shape"""
    if hasattr(matrix, 'tocsr'):
        m = matrix.tocsr()
        if len(m.shape) != 2:
            raise ValueError('matrix must be 2-D')
        return (int(m.shape[0]), int(m.shape[1]), np.asarray(m.indptr).astype(np.int64).reshape(-1),
                np.asarray(m.indices).astype(np.int64).reshape(-1), np.asarray(m.data).reshape(-1))
    a = np.asarray(matrix)
    if a.ndim != 2:
        raise ValueError('matrix must be 2-D')
    if a.dtype.kind == 'c':
        raise NotImplementedError('complex coefficients')
    a = a.astype(np.float64)
    rows, cols = np.nonzero(a)                         # row-major: ascending columns inside a row; NaN is non-zero
    row_ptr = np.zeros(a.shape[0] + 1, dtype=np.int64)
    np.cumsum(np.bincount(rows, minlength=a.shape[0]), out=row_ptr[1:])
    return a.shape[0], a.shape[1], row_ptr, cols.astype(np.int64), a[rows, cols]


def _mix_rows_checked(matrix, offset, n, dtype):
    """mix_rows_arguments with the number of input rows in front"""
    n, dtype = int(n), np.dtype(dtype)
    _real_dtype(dtype)
    rows_out, rows_in, row_ptr, col, val = _mix_rows_csr(matrix)
    if np.iscomplexobj(val):
        raise NotImplementedError('complex coefficients')
    val = np.ascontiguousarray(val, dtype=np.float64)
    if rows_out < 1:
        raise ValueError('rows_out < 1')
    if rows_in < 1:
        raise ValueError('rows_in < 1')
    if rows_out > 2**31 - 1 or rows_in > 2**31 - 1:
        raise ValueError('more than 2**31 - 1 rows')
    if n < 0:
        raise ValueError('n < 0')
    if (len(row_ptr) != rows_out + 1 or row_ptr[0] != 0 or np.any(np.diff(row_ptr) < 0)
            or row_ptr[-1] != len(col) or len(val) != len(col)):
        raise ValueError('row_ptr is not non-decreasing from 0')
    if offset is None:
        offset = np.zeros(rows_out, dtype=np.float64)
    else:
        offset = np.ascontiguousarray(offset, dtype=np.float64).reshape(-1)
        if len(offset) != rows_out:
            raise ValueError('offset: one per output row')
    for r in range(rows_out):
        c, v = col[row_ptr[r]:row_ptr[r + 1]], val[row_ptr[r]:row_ptr[r + 1]]
        bad = np.flatnonzero((c < 0) | (c >= rows_in))
        rising = np.flatnonzero(np.diff(c) <= 0)
        if len(bad) and (not len(rising) or bad[0] <= rising[0] + 1):
            raise ValueError(f'row {r}: column {int(c[bad[0]])} is out of range')
        if len(rising):
            raise ValueError(f'row {r}: columns are not ascending')
        bad = np.flatnonzero(~np.isfinite(v))
        if len(bad):
            raise ValueError(f'row {r}: coefficient ({r}, {int(c[bad[0]])}) is not finite')
        if not np.isfinite(offset[r]):
            raise ValueError(f'row {r}: offset is not finite')
    keep = val != 0.0                                  # a zero is no term, stored or not
    kept = np.zeros(len(val) + 1, dtype=np.int64)
    np.cumsum(keep, out=kept[1:])
    return rows_in, np.ascontiguousarray(kept[row_ptr]), col[keep].astype(np.int32), val[keep], offset, n, dtype


def mix_rows_arguments(matrix, offset, n, dtype=np.float64):
    """the arguments of a MixRowsPlan, checked on the host -> (row_ptr int64, col int32, val float64: the CSR form of
    the matrix's TERMS, its non-zero entries; offset float64, one per output row; n; dtype).  `matrix`: a 2-D
    array-like, or an object with `.tocsr()` (scipy.sparse).  ValueError / NotImplementedError as MixRowsPlan lists
    them.  Needs no device."""
    return _mix_rows_checked(matrix, offset, n, dtype)[1:]


def mix_rows_reads(row_ptr, col) -> int:
    """the sum over tiles of MIX_TILE_ROWS consecutive output rows of the number of input rows the tile has a term on
    (wfk_mix_rows_reads, computed on the host): the kernel reads that many rows of n samples"""
    row_ptr, col = np.asarray(row_ptr), np.asarray(col)
    return sum(len(np.unique(col[row_ptr[o]:row_ptr[min(o + MIX_TILE_ROWS, len(row_ptr) - 1)]]))
               for o in range(0, len(row_ptr) - 1, MIX_TILE_ROWS))


class MixRowsPlan(_Handle):
    """y[o] = sum over the terms (c, M[o, c] != 0) of row o, in ascending c, of x[c] * M[o, c], plus offset[o], per
    sample, for rows_in rows of n float64 / float32 samples -> rows_out rows of the same dtype (in float64, product and
    sum each rounded, a float32 result rounded once; wfk_mix_rows_plan_create).  `.rows_out`, `.rows_in`, `.nnz` (the
    terms), `.reads` (mix_rows_reads).  ValueError before any device work: `matrix must be 2-D`, `rows_out < 1`,
    `rows_in < 1`, `n < 0`, `offset: one per output row`, `row r: column c is out of range`, `row r: columns are not
    ascending`, `row r: coefficient (r, c) is not finite`, `row r: offset is not finite`, `row_ptr is not
    non-decreasing from 0`, `dtype must be float64 or float32` (NotImplementedError for a complex one)."""
    _destroy = 'wfk_mix_rows_plan_destroy'

    def __init__(self, matrix, offset, n: int, dtype=np.float64):
        (self.rows_in, self.row_ptr, self.col, self.val, self.offset, self.n,
         self.dtype) = _mix_rows_checked(matrix, offset, n, dtype)
        self.rows_out, self.nnz = len(self.row_ptr) - 1, len(self.col)
        self.reads = mix_rows_reads(self.row_ptr, self.col)
        check(lib().wfk_mix_rows_plan_create(self.n, self.rows_out, self.rows_in, _KIND_OF[self.dtype],
                                             self.row_ptr.ctypes.data, self.col.ctypes.data, self.val.ctypes.data,
                                             self.offset.ctypes.data, C.byref(self._h)))

    def apply(self, in_ptr, in_stride, out_ptr, out_stride, stream=0):
        check(lib().wfk_mix_rows_apply(self._h, in_ptr, in_stride, out_ptr, out_stride, stream))

    def library_reads(self) -> int:
        return int(lib().wfk_mix_rows_reads(self._h))

    def kernel_name(self) -> str:
        return lib().wfk_mix_rows_kernel_name(self._h).decode()


MIX_DAC_TILE_ROWS = 4      # WFK_MIX_DAC_TILE_ROWS


def mix_dac_arguments(matrix, mix_offset, gain, dac_offset, n, bits=16, shift=0, interleave=1, dtype=np.float64):
    """the arguments of a MixDacPlan, checked on the host: mix_rows_arguments(matrix, mix_offset, n, dtype), then
    dac_rows_arguments(gain, dac_offset, n, bits, shift, interleave, dtype) for one gain and offset per OUTPUT row of
    the matrix -> (rows_in, row_ptr, col, val, mix_offset, gain, dac_offset, n, bits, shift, interleave, dtype).
    ValueError / NotImplementedError as the two list them, the mix's first.  Needs no device."""
    rows_in, row_ptr, col, val, mix_offset, n, dtype = _mix_rows_checked(matrix, mix_offset, n, dtype)
    gain, dac_offset, n, bits, shift, interleave, dtype = dac_rows_arguments(gain, dac_offset, n, bits, shift,
                                                                             interleave, dtype)
    if len(gain) != len(row_ptr) - 1:
        raise ValueError(f'{len(gain)} gains for {len(row_ptr) - 1} output rows')
    return rows_in, row_ptr, col, val, mix_offset, gain, dac_offset, n, bits, shift, interleave, dtype


def mix_dac_reads(row_ptr, col) -> int:
    """mix_rows_reads at the fused kernel's tile height, MIX_DAC_TILE_ROWS (wfk_mix_dac_reads, computed on the host)"""
    row_ptr, col = np.asarray(row_ptr), np.asarray(col)
    return sum(len(np.unique(col[row_ptr[o]:row_ptr[min(o + MIX_DAC_TILE_ROWS, len(row_ptr) - 1)]]))
               for o in range(0, len(row_ptr) - 1, MIX_DAC_TILE_ROWS))


class MixDacPlan(_Handle):
    """DacRowsPlan(gain, dac_offset, ...) on what MixRowsPlan(matrix, mix_offset, ...) gives, in ONE kernel and bit for
    bit -- codes and counts -- without the float rows between them (wfk_mix_dac_plan_create): rows_in rows of n float64 /
    float32 samples -> `.out_rows` = rows_out // interleave rows of `.out_n` = interleave * n int16 codes.  `.rows_out`,
    `.rows_in`, `.nnz`, `.reads` (mix_dac_reads), `.lo` / `.hi`.  ValueError before any device work: what MixRowsPlan
    and DacRowsPlan list, and a number of gains other than rows_out."""
    _destroy = 'wfk_mix_dac_plan_destroy'

    def __init__(self, matrix, mix_offset, gain, dac_offset, n: int, bits: int = 16, shift: int = 0,
                 interleave: int = 1, dtype=np.float64):
        (self.rows_in, self.row_ptr, self.col, self.val, self.mix_offset, self.gain, self.dac_offset, self.n, self.bits,
         self.shift, self.interleave, self.dtype) = mix_dac_arguments(matrix, mix_offset, gain, dac_offset, n, bits,
                                                                      shift, interleave, dtype)
        self.rows_out, self.nnz = len(self.row_ptr) - 1, len(self.col)
        self.reads = mix_dac_reads(self.row_ptr, self.col)
        self.lo, self.hi = -2**(self.bits - 1), 2**(self.bits - 1) - 1
        self.out_rows, self.out_n = self.rows_out // self.interleave, self.interleave * self.n
        check(lib().wfk_mix_dac_plan_create(self.n, self.rows_out, self.rows_in, _KIND_OF[self.dtype],
                                            self.row_ptr.ctypes.data, self.col.ctypes.data, self.val.ctypes.data,
                                            self.mix_offset.ctypes.data, self.gain.ctypes.data,
                                            self.dac_offset.ctypes.data, self.bits, self.shift, self.interleave,
                                            C.byref(self._h)))

    def apply(self, in_ptr, in_stride, out_ptr, out_stride, counts_ptr=None, stream=0):
        """counts_ptr: None, or rows_out * 3 int64 on the device, overwritten with [below, above, nan] per mix row"""
        check(lib().wfk_mix_dac_apply(self._h, in_ptr, in_stride, out_ptr, out_stride, counts_ptr, stream))

    def library_reads(self) -> int:
        return int(lib().wfk_mix_dac_reads(self._h))

    def span(self) -> int:
        """the codes of one row a workgroup covers"""
        return int(lib().wfk_mix_dac_span(self._h))

    def kernel_name(self, counts: bool = False) -> str:
        return lib().wfk_mix_dac_kernel_name(self._h, 1 if counts else 0).decode()


CURVE_MAX_KNOTS = 1024     # WFK_CURVE_MAX_KNOTS


def _curve_rows_list(name, rows):
    """`rows` -- a list of 1-D array-likes (ragged), a 2-D array, or ONE 1-D array-like -- as a list of float64 1-D
    arrays; ValueError for anything else, NotImplementedError for complex values"""
    if isinstance(rows, np.ndarray) and rows.dtype != object:
        if rows.ndim not in (1, 2):
            raise ValueError(f'{name}: a list of 1-D arrays, a 2-D array or one 1-D array')
        rows = [rows] if rows.ndim == 1 else list(rows)
    else:
        rows = list(rows)
        if rows and all(np.ndim(r) == 0 for r in rows):
            rows = [rows]
    out = []
    for r, a in enumerate(rows):
        a = np.asarray(a)
        if a.ndim != 1:
            raise ValueError(f'row {r}: {name} is not 1-D')
        if a.dtype.kind == 'c':
            raise NotImplementedError('complex curves')
        out.append(np.ascontiguousarray(a, dtype=np.float64))
    return out


def _curve_ends(name, value, default, batch):
    """left / right: None (the row's own end value), a scalar (every row) or one value per row; any double"""
    if value is None:
        return np.array(default, dtype=np.float64)
    v = np.asarray(value, dtype=np.float64)
    if v.ndim == 0:
        return np.full(batch, float(v))
    v = np.ascontiguousarray(v).reshape(-1)
    if len(v) != batch:
        raise ValueError(f'{len(v)} values of {name} for {batch} rows')
    return v


def curve_rows_arguments(xp_rows, fp_rows, left=None, right=None, batch=None, n=0, dtype=np.float64):
    """the arguments of a CurveRowsPlan, checked on the host -> (knot_ptr int64 [batch + 1], xp, fp float64 [knot_ptr[-1]]:
    the rows' knots and values back to back; left, right float64 [batch]; n; dtype).  `xp_rows` / `fp_rows`: a list of
    1-D arrays (rows may differ in length), a 2-D array, or one 1-D pair that every one of `batch` rows shares.
    ValueError / NotImplementedError as CurveRowsPlan lists them.  Needs no device."""
    n, dtype = int(n), np.dtype(dtype)
    _real_dtype(dtype)
    xs, fs = _curve_rows_list('xp', xp_rows), _curve_rows_list('fp', fp_rows)
    if len(xs) != len(fs):
        raise ValueError(f'{len(xs)} rows of xp and {len(fs)} rows of fp')
    if batch is None:
        batch = len(xs)
    batch = int(batch)
    if batch < 1:
        raise ValueError('no rows')
    if len(xs) == 1 and batch > 1:
        xs, fs = xs * batch, fs * batch
    if len(xs) != batch:
        raise ValueError(f'{len(xs)} curves for {batch} rows')
    if n < 0:
        raise ValueError('n >= 0')
    for r, (x, f) in enumerate(zip(xs, fs)):
        if len(x) != len(f):
            raise ValueError(f'row {r}: {len(x)} knots and {len(f)} values')
        if len(x) < 2:
            raise ValueError(f'row {r}: fewer than 2 knots')
        if len(x) > CURVE_MAX_KNOTS:
            raise ValueError(f'row {r}: more than {CURVE_MAX_KNOTS} knots')
        bad = np.flatnonzero(~np.isfinite(x))
        rising = np.flatnonzero(~(x[1:] > x[:-1])) + 1            # (a NaN knot fails the comparison on both sides)
        if len(bad) and (not len(rising) or bad[0] <= rising[0]):
            raise ValueError(f'row {r}: knot {int(bad[0])} is not finite')
        if len(rising):
            raise ValueError(f'row {r}: knots are not strictly increasing at {int(rising[0])}')
        bad = np.flatnonzero(~np.isfinite(f))
        if len(bad):
            raise ValueError(f'row {r}: value {int(bad[0])} is not finite')
    knot_ptr = np.zeros(batch + 1, dtype=np.int64)
    np.cumsum([len(x) for x in xs], out=knot_ptr[1:])
    left = _curve_ends('left', left, [f[0] for f in fs], batch)
    right = _curve_ends('right', right, [f[-1] for f in fs], batch)
    return knot_ptr, np.concatenate(xs), np.concatenate(fs), left, right, n, dtype


class CurveRowsPlan(_Handle):
    """y[r] = np.interp(x[r], xp[r], fp[r], left[r], right[r]), bit for bit, for `batch` rows of n float64 / float32
    samples, every row its own curve of 2 .. CURVE_MAX_KNOTS knots (in float64: a rounded difference, product and sum,
    no fused multiply-add; a float32 result rounded once; a NaN sample stays that NaN; wfk_curve_rows_plan_create).
    `.knots`: the knots per row; `.spans`: the spans a workgroup walks.  ValueError before any device work: `no rows`,
    `N curves for B rows`, `n >= 0`, `row r: K knots and M values`, `row r: fewer than 2 knots`, `row r: more than 1024
    knots`, `row r: knot j is not finite`, `row r: knots are not strictly increasing at j`, `row r: value j is not
    finite`, `dtype must be float64 or float32` (NotImplementedError for a complex one)."""
    _destroy = 'wfk_curve_rows_plan_destroy'

    def __init__(self, xp_rows, fp_rows, n: int, batch=None, left=None, right=None, dtype=np.float64):
        (self.knot_ptr, self.xp, self.fp, self.left, self.right, self.n,
         self.dtype) = curve_rows_arguments(xp_rows, fp_rows, left, right, batch, n, dtype)
        self.batch = len(self.knot_ptr) - 1
        self.knots = np.diff(self.knot_ptr)
        check(lib().wfk_curve_rows_plan_create(self.n, self.batch, _KIND_OF[self.dtype], self.knot_ptr.ctypes.data,
                                               self.xp.ctypes.data, self.fp.ctypes.data, self.left.ctypes.data,
                                               self.right.ctypes.data, C.byref(self._h)))
        self.spans = int(lib().wfk_curve_rows_spans(self._h))

    def apply(self, in_ptr, in_stride, out_ptr, out_stride, counts_ptr=None, stream=0):
        """counts_ptr: None, or batch * 3 int64 on the device, overwritten with [below, above, nan] per row"""
        check(lib().wfk_curve_rows_apply(self._h, in_ptr, in_stride, out_ptr, out_stride, counts_ptr, stream))

    def kernel_name(self, counts: bool = False) -> str:
        return lib().wfk_curve_rows_kernel_name(self._h, 1 if counts else 0).decode()


def curve_iir_dac_arguments(xp_rows, fp_rows, sections_per_row, gain, offset, n, bits=16, shift=0, left=None, right=None,
                            batch=None, dtype=np.float64, packed=None):
    """the arguments of a CurveIirDacPlan, checked on the host: the curve's rules first (curve_rows_arguments), then the
    converter's (dac_rows_arguments, interleave 1), then the cascades' (pack_sections_rows), each with its own texts ->
    (curve: curve_rows_arguments' tuple, dac: dac_rows_arguments' tuple, packed: pack_sections_rows' tuple).  The number
    of curves decides the rows: `N gains for B rows`, `N cascades for B rows`.  Needs no device."""
    curve = curve_rows_arguments(xp_rows, fp_rows, left, right, batch, n, dtype)
    rows = len(curve[0]) - 1
    dac = dac_rows_arguments(gain, offset, n, bits, shift, 1, dtype)
    if len(dac[0]) != rows:
        raise ValueError(f'{len(dac[0])} gains for {rows} rows')
    packed = pack_sections_rows(sections_per_row) if packed is None else packed
    if packed[1].shape[0] != rows:
        raise ValueError(f'{packed[1].shape[0]} cascades for {rows} rows')
    return curve, dac, packed


class CurveIirDacPlan(_Handle):
    """CurveRowsPlan(xp_rows, fp_rows, n, batch, left, right, dtype) followed by IirRowsDacPlan(sections_per_row, gain,
    offset, n, bits, shift, dtype), bit for bit -- codes, the converter's counts, the curve's `beyond` and the final
    states -- in one kernel, 'iir_rows_curve_dac<T,NSEC,ORD>', without the float rows between them
    (wfk_curve_iir_dac_plan_create).  One curve, one cascade and one gain and offset per row; the errors of the three
    parents -- the curve's first, then the converter's, then the cascades' -- before any device work
    (`curve_iir_dac_arguments`).  `state_dim`, `own_orders`, `orders` as IirRowsPlan; `.lo` / `.hi`: the rails;
    `.knots`: the knots per row."""
    _destroy = 'wfk_curve_iir_dac_plan_destroy'

    def __init__(self, xp_rows, fp_rows, sections_per_row, gain, offset, n: int, bits: int = 16, shift: int = 0,
                 left=None, right=None, batch=None, dtype=np.float64, packed=None):
        curve, dac, packed = curve_iir_dac_arguments(xp_rows, fp_rows, sections_per_row, gain, offset, n, bits, shift,
                                                     left, right, batch, dtype, packed)
        self.knot_ptr, self.xp, self.fp, self.left, self.right, self.n, self.dtype = curve
        self.gain, self.offset, _, self.bits, self.shift, _, _ = dac
        orders, bm, am, self.own_orders = packed
        self.batch, self.orders, self.knots = len(self.knot_ptr) - 1, orders, np.diff(self.knot_ptr)
        self.lo, self.hi = -2**(self.bits - 1), 2**(self.bits - 1) - 1
        bm, am = np.ascontiguousarray(bm), np.ascontiguousarray(am)
        check(lib().wfk_curve_iir_dac_plan_create(len(orders), orders.ctypes.data, bm.ctypes.data, am.ctypes.data,
                                                  self.n, self.batch, _KIND_OF[self.dtype], self.knot_ptr.ctypes.data,
                                                  self.xp.ctypes.data, self.fp.ctypes.data, self.left.ctypes.data,
                                                  self.right.ctypes.data, self.gain.ctypes.data,
                                                  self.offset.ctypes.data, self.bits, self.shift, C.byref(self._h)))
        self.state_dim = int(orders.sum())

    def apply(self, in_ptr, in_stride, out_ptr, out_stride, counts_ptr=None, beyond_ptr=None, zi_ptr=None,
              zf_ptr=None, initial_ptr=None, stream=0):
        """counts_ptr / beyond_ptr: None, or batch * 3 int64 on the device, overwritten with the converter's / the
        curve's [below, above, nan] per row; initial_ptr: device array of `batch` doubles (one level per row) or None"""
        check(lib().wfk_curve_iir_dac_apply(self._h, in_ptr, in_stride, out_ptr, out_stride, counts_ptr, beyond_ptr,
                                            zi_ptr, zf_ptr, initial_ptr, stream))

    def apply_shared_in(self, in_ptr, out_ptr, out_stride, counts_ptr=None, beyond_ptr=None, zi_ptr=None, zf_ptr=None,
                        initial_ptr=None, stream=0):
        """every row reads the SAME n input samples at `in_ptr`"""
        check(lib().wfk_curve_iir_dac_apply_shared_in(self._h, in_ptr, out_ptr, out_stride, counts_ptr, beyond_ptr,
                                                      zi_ptr, zf_ptr, initial_ptr, stream))

    def kernel_name(self) -> str:
        return lib().wfk_curve_iir_dac_kernel_name(self._h).decode()


class ChainCurveIirDacPlan(_Handle):
    """sampler -> per-row curve -> per-row IIR -> DAC codes for every channel of `prog` on `grid`
    (wfk_chain_curve_iir_dac_*): Plan(prog, grid) (float64), CurveRowsPlan in place and IirRowsDacPlan, bit for bit.
    Fused where ChainIirRowsDacPlan is -- 'iir_rows_sampled_curve_dac<f64,NSEC,ORD>' on fine grids,
    'iir_rows_short_curve_dac<f64,NSEC,ORD>' at AWG rates: 2 B per sample of HBM traffic -- but for curves whose knots
    do not fit next to the lean fill's LDS; everything else (`why_not`) runs the sampler into a float64 scratch the
    caller lends, then 'iir_rows_curve_dac<f64,NSEC,ORD>'.  The errors of `curve_iir_dac_arguments`, in its order."""
    _destroy = 'wfk_chain_curve_iir_dac_plan_destroy'

    def __init__(self, prog: Program, grid: wfk_grid, xp_rows, fp_rows, sections_per_row, gain, offset, bits: int = 16,
                 shift: int = 0, left=None, right=None, packed=None):
        curve, dac, packed = curve_iir_dac_arguments(xp_rows, fp_rows, sections_per_row, gain, offset, int(grid.n), bits,
                                                     shift, left, right, prog.n_channels, np.float64, packed)
        self.knot_ptr, self.xp, self.fp, self.left, self.right, self.n, _ = curve
        self.gain, self.offset, _, self.bits, self.shift, _, _ = dac
        orders, bm, am, self.own_orders = packed
        self.prog, self.grid, self.n_channels, self.orders = prog, grid, prog.n_channels, orders
        self.knots = np.diff(self.knot_ptr)
        self.lo, self.hi = -2**(self.bits - 1), 2**(self.bits - 1) - 1
        bm, am = np.ascontiguousarray(bm), np.ascontiguousarray(am)
        check(lib().wfk_chain_curve_iir_dac_plan_create(C.byref(prog.struct), C.byref(grid), len(orders),
                                                        orders.ctypes.data, bm.ctypes.data, am.ctypes.data,
                                                        self.knot_ptr.ctypes.data, self.xp.ctypes.data,
                                                        self.fp.ctypes.data, self.left.ctypes.data,
                                                        self.right.ctypes.data, self.gain.ctypes.data,
                                                        self.offset.ctypes.data, self.bits, self.shift, C.byref(self._h)))
        self.state_dim = int(orders.sum())
        self.fused = bool(lib().wfk_chain_curve_iir_dac_is_fused(self._h))
        self.why_not = lib().wfk_chain_curve_iir_dac_unfused_reason(self._h).decode()

    def launch(self, out_ptr, out_stride, counts_ptr=None, beyond_ptr=None, scratch_ptr=None, scratch_stride=0,
               zi_ptr=None, zf_ptr=None, initial_ptr=None, stream=0):
        """counts_ptr / beyond_ptr: None, or n_channels * 3 int64 on the device, overwritten with the converter's / the
        curve's [below, above, nan]; scratch_ptr: n_channels float64 rows `scratch_stride` apart, which an unfused plan
        needs and a fused one does not touch"""
        check(lib().wfk_chain_curve_iir_dac_launch(self._h, out_ptr, out_stride, counts_ptr, beyond_ptr, scratch_ptr,
                                                   scratch_stride, zi_ptr, zf_ptr, initial_ptr, stream))

    def kernel_name(self) -> str:
        """'iir_rows_sampled_curve_dac<f64,NSEC,ORD>', 'iir_rows_short_curve_dac<f64,NSEC,ORD>', or the sampler's
        kernels and 'iir_rows_curve_dac<f64,NSEC,ORD>' joined with ' + '"""
        return lib().wfk_chain_curve_iir_dac_kernel_name(self._h).decode()

    def table_bytes(self) -> int:
        return int(lib().wfk_chain_curve_iir_dac_table_bytes(self._h))


class ExtractRowsPlan(_Handle):
    """ker[r] = the reference's extractKernel of (sig_in[r], sig_out[r]) for `batch` rows of n doubles
    (wfk_extract_rows_plan_create): spectral ratio, centred inverse transform, `taps` (None: no smoothing) convolved
    in 'same' mode, `skip` samples cut at each end; `.k` = max(n - 2 skip, 0) samples per result row.
    `shared_input`: one sig_in row for all rows.  ValueError before any device work: n < 1, batch < 1, skip < 0,
    more taps than samples, taps that are not a finite 1-D array."""
    _destroy = 'wfk_extract_rows_plan_destroy'

    def __init__(self, n: int, batch: int, taps=None, skip: int = 0, shared_input: bool = False):
        self.n, self.batch, self.skip = int(n), int(batch), int(skip)
        self.shared_input = bool(shared_input)
        if self.n < 1 or self.batch < 1:
            raise ValueError('n >= 1 and batch >= 1')
        if self.skip < 0:
            raise ValueError('skip must not be negative (the reference slices ker[skip:len(ker) - skip]; '
                             'a negative skip is refused here)')
        if taps is not None:
            taps = np.ascontiguousarray(taps, dtype=np.float64)
            if taps.ndim != 1 or not np.all(np.isfinite(taps)):
                raise ValueError('taps must be a 1-D array of finite values')
            if len(taps) > self.n:
                raise ValueError(f'{len(taps)} smoothing taps for rows of {self.n} samples: the reference returns '
                                 f'{len(taps)} samples there, rows keep their length here, so it is refused')
            if len(taps) == 0:
                taps = None
        self.taps = taps
        self.k = max(self.n - 2 * self.skip, 0)
        check(lib().wfk_extract_rows_plan_create(self.n, self.batch, 1 if self.shared_input else self.batch,
                                                 None if taps is None else taps.ctypes.data,
                                                 0 if taps is None else len(taps), self.skip, C.byref(self._h)))

    def apply(self, sig_in_ptr, in_stride, sig_out_ptr, out_sig_stride, ker_ptr, ker_stride, stream=0):
        check(lib().wfk_extract_rows_apply(self._h, sig_in_ptr, in_stride, sig_out_ptr, out_sig_stride, ker_ptr,
                                           ker_stride, stream))

    def kernel_name(self) -> str:
        return lib().wfk_extract_rows_kernel_name(self._h).decode()


IN_F64, IN_F32, IN_I16 = 0, 1, 4
DEMOD_IN_KIND = {np.dtype(np.float64): IN_F64, np.dtype(np.float32): IN_F32, np.dtype(np.int16): IN_I16}


class DemodPlan(_Handle):
    """out[s, j] = sum_k x[s, k] * e[k, j]: real traces (shots, >= N) of float64 / float32 / int16 times a complex
    (N, nf) matrix, fp64 on the device; `e` is uploaded once."""
    _destroy = 'wfk_demod_plan_destroy'

    def __init__(self, e, dtype=np.float64):
        e = np.ascontiguousarray(e, dtype=np.complex128)
        if e.ndim != 2 or e.shape[0] < 1 or e.shape[1] < 1:
            raise ValueError('e must be a non-empty (N, nf) complex matrix')
        self.dtype = np.dtype(dtype)
        if self.dtype not in DEMOD_IN_KIND:
            raise ValueError('trace dtype must be float64, float32 or int16')
        self.n, self.nf = int(e.shape[0]), int(e.shape[1])
        check(lib().wfk_demod_plan_create(e.ctypes.data, self.n, self.nf, DEMOD_IN_KIND[self.dtype],
                                          C.byref(self._h)))

    def apply(self, x_ptr, n_shots, x_stride, out_ptr, out_stride, stream=0):
        check(lib().wfk_demod_apply(self._h, x_ptr, n_shots, x_stride, out_ptr, out_stride, stream))

    def kernel_name(self, n_shots: int) -> str:
        return lib().wfk_demod_kernel_name(self._h, n_shots).decode()


def bdemod_arguments(e, bin, start=0, bins=None, dtype=np.float64):
    """the arguments of a BinnedDemodPlan, checked on the host -> (e: a C-contiguous (N, nf) complex128 array, start,
    bin, bins, dtype); `bins=None` means all that fit, (N - start) // bin.  ValueError: a matrix that is not a non-empty
    (N, nf), a trace dtype that is not float64, float32 or int16, `bin >= 1`, `start >= 0`, `bins >= 1`, start + bins *
    bin > N, bins * nf above 2^31 - 1, an entry of the rows [start, start + bins * bin) of e that is not finite (its
    index is named).  Needs no device."""
    e = np.asarray(e)
    if e.ndim != 2 or e.shape[0] < 1 or e.shape[1] < 1:
        raise ValueError('the matrix must be (N, nf) with N >= 1 and nf >= 1, got shape %s' % (e.shape,))
    dtype = np.dtype(dtype)
    if dtype not in DEMOD_IN_KIND:
        raise ValueError('trace dtype must be float64, float32 or int16, got %s' % dtype)
    e = np.ascontiguousarray(e, dtype=np.complex128)
    n, nf = e.shape
    bin, start = int(bin), int(start)
    if bin < 1:
        raise ValueError('binned demodulator: bin >= 1, got %d' % bin)
    if start < 0:
        raise ValueError('binned demodulator: start >= 0, got %d' % start)
    bins = max(n - start, 0) // bin if bins is None else int(bins)
    if bins < 1:
        raise ValueError('binned demodulator: bins >= 1, got %d (N = %d, start = %d, bin = %d)' % (bins, n, start, bin))
    if start + bins * bin > n:
        raise ValueError('binned demodulator: start + bins * bin = %d exceeds N = %d' % (start + bins * bin, n))
    if bins * nf > 2**31 - 1:
        raise ValueError('binned demodulator: bins * nf exceeds 2^31 - 1')
    used = e[start:start + bins * bin]
    bad = np.argwhere(~(np.isfinite(used.real) & np.isfinite(used.imag)))
    if len(bad):
        raise ValueError('binned demodulator: e[%d, %d] is not finite' % (start + int(bad[0][0]), int(bad[0][1])))
    return e, start, bin, bins, dtype


def bdemod_bin_groups(n_shots: int, n_freq: int, bins: int) -> int:
    """workgroups along the bin axis for a block of n_shots (wfk_bdemod_bin_groups): the shape alone, no device"""
    return int(lib().wfk_bdemod_bin_groups(n_shots, n_freq, bins))


class BinnedDemodPlan(_Handle):
    """out[s, w, j] = the sum over bin w = [start + w bin, start + (w + 1) bin) of x[s, k] * e[k, j]: real traces
    (shots, >= N) of float64 / float32 / int16 times a complex (N, nf) matrix, per time bin, fp64 on the device
    (wfk_bdemod_plan_create); the used rows of `e` are uploaded once."""
    _destroy = 'wfk_bdemod_plan_destroy'

    def __init__(self, e, bin, start=0, bins=None, dtype=np.float64):
        e, self.start, self.bin, self.bins, self.dtype = bdemod_arguments(e, bin, start, bins, dtype)
        self.n, self.nf = int(e.shape[0]), int(e.shape[1])
        check(lib().wfk_bdemod_plan_create(e.ctypes.data, self.n, self.nf, DEMOD_IN_KIND[self.dtype], self.start,
                                           self.bin, self.bins, C.byref(self._h)))

    def apply(self, x_ptr, n_shots, x_stride, out_ptr, out_stride, stream=0):
        check(lib().wfk_bdemod_apply(self._h, x_ptr, n_shots, x_stride, out_ptr, out_stride, stream))

    def kernel_name(self, n_shots: int) -> str:
        """'bdemod_tile<T,NB> groups=G'"""
        return lib().wfk_bdemod_kernel_name(self._h, n_shots).decode()


def avg_arguments(n_points, steps, dtype):
    """the arguments of an AvgPlan, checked on the host -> (n_points, steps, dtype).  ValueError: `n_points >= 1`,
    `steps >= 1`, a trace dtype that is not float64, float32 or int16.  Needs no device."""
    n_points, steps, dtype = int(n_points), int(steps), np.dtype(dtype)
    if n_points < 1:
        raise ValueError('trace averager: n_points >= 1, got %d' % n_points)
    if steps < 1:
        raise ValueError('trace averager: steps >= 1, got %d' % steps)
    if dtype not in DEMOD_IN_KIND:
        raise ValueError('trace dtype must be float64, float32 or int16, got %s' % dtype)
    return n_points, steps, dtype


class AvgPlan(_Handle):
    """sum[g, c] = the sum over the block's shots s with (first + s) mod steps == g of x[s, c], and the same of the
    squares: real traces (shots, >= n_points) of float64 / float32 / int16 into (steps, n_points) int64 (int16 codes,
    exact) or float64 sums on the device (wfk_avg_plan_create); the plan owns the workspace of a split launch."""
    _destroy = 'wfk_avg_plan_destroy'

    def __init__(self, n_points: int, steps: int = 1, dtype=np.int16):
        self.n, self.steps, self.dtype = avg_arguments(n_points, steps, dtype)
        self.sum_dtype = np.dtype(np.int64 if self.dtype == np.dtype(np.int16) else np.float64)
        check(lib().wfk_avg_plan_create(self.n, self.steps, DEMOD_IN_KIND[self.dtype], C.byref(self._h)))

    def apply(self, x_ptr, n_shots, x_stride, first, sum_ptr, sum_stride, sumsq_ptr=None, sumsq_stride=0,
              accumulate=False, stream=0):
        check(lib().wfk_avg_apply(self._h, x_ptr, n_shots, x_stride, first, sum_ptr, sum_stride, sumsq_ptr,
                                  sumsq_stride, 1 if accumulate else 0, stream))

    def splits(self, n_shots: int, first: int = 0) -> int:
        return int(lib().wfk_avg_splits(self._h, n_shots, first))

    def kernel_name(self, n_shots: int, sumsq: bool = True) -> str:
        return lib().wfk_avg_kernel_name(self._h, n_shots, 1 if sumsq else 0).decode()


STATES_MAX_TONES, STATES_MAX_STATES = 1024, 8      # WFK_STATES_MAX_TONES / WFK_STATES_MAX_STATES


def states_bits(n_states: int) -> int:
    """bits a tone takes in a shot's word: 1 for two states, 2 up to four, 3 up to eight"""
    return 1 if n_states <= 2 else 2 if n_states <= 4 else 3


def states_arguments(centres, steps=1):
    """the arguments of a StatesPlan, checked on the host -> (centres: a C-contiguous (n_tones, n_states) complex128
    array, steps).  ValueError: centres that are not 2-D, n_states outside [2, 8], n_tones outside [1, 1024],
    `steps >= 1`, steps * n_tones * (n_states + 1) above 2^31 - 1, a tone without a finite centre (NaN centres pad a
    tone with fewer states; the tone is named).  Needs no device."""
    centres = np.asarray(centres)
    if centres.ndim != 2:
        raise ValueError('state discriminator: centres must be (n_tones, n_states), got shape %s' % (centres.shape,))
    centres = np.ascontiguousarray(centres, dtype=np.complex128)
    nf, k = centres.shape
    steps = int(steps)
    if not 2 <= k <= STATES_MAX_STATES:
        raise ValueError('state discriminator: n_states must lie in [2, %d], got %d' % (STATES_MAX_STATES, k))
    if not 1 <= nf <= STATES_MAX_TONES:
        raise ValueError('state discriminator: n_tones must lie in [1, %d], got %d' % (STATES_MAX_TONES, nf))
    if steps < 1:
        raise ValueError('state discriminator: steps >= 1, got %d' % steps)
    if steps * nf * (k + 1) > 2**31 - 1:
        raise ValueError('state discriminator: steps * n_tones * (n_states + 1) exceeds 2^31 - 1')
    bad = np.flatnonzero(~(np.isfinite(centres.real) & np.isfinite(centres.imag)).any(axis=1))
    if len(bad):
        raise ValueError('tone %d: no finite centre' % int(bad[0]))
    return centres, steps


class StatesPlan(_Handle):
    """label[s, j] = the nearest of tone j's centres to the IQ point x[s, j] (complex128 rows, squared distance in
    double without a fused multiply-add, ties to the lowest state, 255 where no centre wins), and from the labels the
    packed words, the per-step counts (steps, n_tones, n_states + 1) and the joint histogram (steps, 2^(n_tones bits)
    + 1), all int64 (wfk_states_plan_create); the plan owns the table of centres."""
    _destroy = 'wfk_states_plan_destroy'

    def __init__(self, centres, steps: int = 1):
        self.centres, self.steps = states_arguments(centres, steps)
        self.nf, self.k = self.centres.shape
        self.bits = states_bits(self.k)
        check(lib().wfk_states_plan_create(self.centres.ctypes.data, self.nf, self.k, self.steps, C.byref(self._h)))

    def apply(self, x_ptr, n_shots, x_stride, first, labels_ptr=None, labels_stride=0, words_ptr=None,
              counts_ptr=None, joint_ptr=None, accumulate=False, stream=0):
        check(lib().wfk_states_apply(self._h, x_ptr, n_shots, x_stride, first, labels_ptr, labels_stride, words_ptr,
                                     counts_ptr, joint_ptr, 1 if accumulate else 0, stream))

    def kernel_name(self, n_shots: int) -> str:
        """'states_block<KT> tile=T counts:lds|global joint:lds|global|none'"""
        return lib().wfk_states_kernel_name(self._h, n_shots).decode()


def probe_brackets(tlist, t):
    """np.interp's bracket of every probe time `t` in the ascending grid `tlist`, as the probe plan uploads it (host
    only, no device): -> (j int64, dx, w) with dx = t - tlist[j], w = tlist[j + 1] - tlist[j]; t outside the grid:
    the first / last index with dx = 0, w = 1; NaN: j = 0, dx = NaN."""
    tlist = np.ascontiguousarray(tlist, dtype=np.float64).reshape(-1)
    t = np.ascontiguousarray(t, dtype=np.float64).reshape(-1)
    j, dx, w = np.empty(len(t), dtype=np.int64), np.empty(len(t)), np.empty(len(t))
    check(lib().wfk_boxprobe_brackets(tlist.ctypes.data, len(tlist), t.ctypes.data, len(t), j.ctypes.data,
                                      dx.ctypes.data, w.ctypes.data))
    return j, dx, w


class BoxProbePlan(_Handle):
    """out[r, q] = np.interp(t[q], tlist, conv[r]), conv[r, i] = gain * sum_{m < pp} y[r, i + c - m] (zero padded):
    the boxcar integral of every row of a (rows, >= n) float64 device array read off at the probe times `t`;
    tlist and t are bracketed on the host and uploaded once."""
    _destroy = 'wfk_boxprobe_plan_destroy'

    def __init__(self, tlist, t, pp: int, c: int, gain: float):
        tlist = np.ascontiguousarray(tlist, dtype=np.float64).reshape(-1)
        t = np.ascontiguousarray(t, dtype=np.float64).reshape(-1)
        self.n, self.nq, self.pp, self.c, self.gain = len(tlist), len(t), int(pp), int(c), float(gain)
        check(lib().wfk_boxprobe_plan_create(tlist.ctypes.data, self.n, t.ctypes.data, self.nq, self.pp, self.c,
                                             self.gain, C.byref(self._h)))

    def apply(self, y_ptr, n_rows, y_stride, out_ptr, out_stride, stream=0):
        check(lib().wfk_boxprobe_apply(self._h, y_ptr, n_rows, y_stride, out_ptr, out_stride, stream))

    def kernel_name(self) -> str:
        return lib().wfk_boxprobe_kernel_name(self._h).decode()


class DeviceBuffer:
    """Raw device allocation through the C-ABI (for callers without torch)."""

    def __init__(self, nbytes: int):
        self.nbytes = int(nbytes)
        p = C.c_void_p()
        check(lib().wfk_malloc(C.byref(p), self.nbytes))
        self.ptr = p.value

    def upload(self, arr: np.ndarray):
        arr = np.ascontiguousarray(arr)
        check(lib().wfk_memcpy_h2d(self.ptr, arr.ctypes.data, arr.nbytes))

    def download(self, shape, dtype) -> np.ndarray:
        out = np.empty(shape, dtype=dtype)
        check(lib().wfk_memcpy_d2h(out.ctypes.data, self.ptr, out.nbytes))
        return out

    def zero(self):
        check(lib().wfk_memset(self.ptr, 0, self.nbytes))

    def close(self):
        if getattr(self, 'ptr', None) and _lib is not None:
            _lib.wfk_free(self.ptr)
            self.ptr = None

    __del__ = close

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()


def sync(stream: int = 0):
    check(lib().wfk_stream_sync(stream))
