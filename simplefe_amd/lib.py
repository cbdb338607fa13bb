"""ctypes binding of libsfe_dsp.so -- the C ABI declared in include/sfe_dsp.h.

The library is the product: there is no Python or CPU fallback.  If the in-tree .so is
missing or fails to load this module raises; if no GPU is usable the create calls fail
with SFE_ENODEV (and SfeError is raised by the wrappers in api.py).
"""
import ctypes as C
import os

HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.path.join(HERE, "libsfe_dsp.so")

SFE_OK, SFE_EINVAL, SFE_ENOMEM, SFE_EHIP, SFE_ENODEV, SFE_ESTATE, SFE_ERANGE = 0, -1, -2, -3, -4, -5, -6
FIR_ALGO_AUTO, FIR_ALGO_DIRECT, FIR_ALGO_FFT = 0, 1, 2
FIR_VARIANT_AUTO, FIR_VARIANT_REGISTER_LOADS, FIR_VARIANT_LDS_DMA, FIR_VARIANT_WAVE_PRIVATE = -1, 0, 1, 2
FIR_VARIANT_NAMES = {-1: "auto", 0: "register loads", 1: "LDS-DMA", 2: "LDS-DMA, wave-private layout"}
RS_RESAMPLE, RS_DECIMATE = 0, 1
RS_ALGO_AUTO, RS_ALGO_DIRECT, RS_ALGO_FFT, RS_ALGO_MFMA = 0, 1, 2, 3
FMT_F32, FMT_U8, FMT_TX10 = 0, 1, 2
VIT_IN_SOFT, VIT_IN_BPSK, VIT_IN_QPSK = 0, 1, 2      # sfe_dsp_vit_*: what d_in holds
POLAR_FM, POLAR_PM, POLAR_AM = 0, 1, 2               # sfe_dsp_polar_*: the law fixed at create
OCC_NONFINITE, OCC_TRUNCATED = 1, 2                  # sfe_dsp_occ_*: the bits of a row's status
REED_OK, REED_UNCORRECTABLE, REED_UPSTREAM = 0, 1, 2 # sfe_dsp_reed_*: a frame's status
LDPC_OK, LDPC_NOT_FINITE, LDPC_UPSTREAM, LDPC_NOT_CONVERGED = 0, 1, 2, 3     # sfe_dsp_ldpc_*: a codeword's status
OFDM_OUT_ZF, OFDM_OUT_MRC = 0, 1                     # sfe_dsp_ofdm_*: out_mode
OFDM_OK, OFDM_NO_ESTIMATE, OFDM_GATED, OFDM_OUT_OF_RANGE = 0, 1, 2, 3        # sfe_dsp_ofdm_*: a burst's status
OFDMMOD_IN_BITS, OFDMMOD_IN_SYMBOLS = 0, 1           # sfe_dsp_ofdmmod_*: in_mode
QAM_MAP, QAM_DEMAP = 0, 1                            # sfe_dsp_qam_plan: direction
FSK_MOD, FSK_DEMOD = 0, 1                            # sfe_dsp_fsk_plan: direction
CRC_OK, CRC_MISMATCH, CRC_UPSTREAM = 0, 1, 2         # sfe_dsp_crc_*: a frame's status


class TimeState(C.Structure):
    _fields_ = [("pos", C.c_int32), ("mu", C.c_float), ("leftover", C.c_int32)]


vp, sz, i32, f32, u32 = C.c_void_p, C.c_size_t, C.c_int, C.c_float, C.c_uint32
fp = C.POINTER(C.c_float)

# name -> (restype, argtypes): every symbol include/sfe_dsp.h declares
SIGNATURES = {
    "sfe_dsp_version": (C.c_char_p, []),
    "sfe_dsp_last_error": (C.c_char_p, []),
    "sfe_dsp_device_count": (i32, [C.POINTER(i32)]),
    "sfe_dsp_set_device": (i32, [i32]),
    "sfe_dsp_get_device": (i32, [C.POINTER(i32)]),
    "sfe_dsp_sync": (i32, [vp]),
    "sfe_dsp_malloc": (i32, [C.POINTER(vp), sz]),
    "sfe_dsp_free": (i32, [vp]),
    "sfe_dsp_host_alloc": (i32, [C.POINTER(vp), sz]),
    "sfe_dsp_host_free": (i32, [vp]),
    "sfe_dsp_memcpy_h2d": (i32, [vp, vp, sz, vp]),
    "sfe_dsp_memcpy_d2h": (i32, [vp, vp, sz, vp]),
    "sfe_dsp_memset": (i32, [vp, i32, sz, vp]),
    "sfe_dsp_timer_create": (i32, [C.POINTER(vp)]),
    "sfe_dsp_timer_start": (i32, [vp, vp]),
    "sfe_dsp_timer_stop": (i32, [vp, vp]),
    "sfe_dsp_timer_elapsed_ms": (i32, [vp, C.POINTER(f32)]),
    "sfe_dsp_timer_destroy": (i32, [vp]),
    "sfe_dsp_synth_fill": (i32, [vp, C.c_uint64, C.c_uint32, C.c_uint32, C.c_uint64, vp]),
    "sfe_dsp_fir_create": (i32, [vp, i32, i32, i32, i32, i32, i32, C.POINTER(vp)]),
    "sfe_dsp_fir_create_per_channel": (i32, [vp, i32, i32, i32, i32, C.POINTER(vp)]),
    "sfe_dsp_fir_plan": (i32, [i32, C.POINTER(i32), C.POINTER(i32), C.POINTER(i32)]),
    "sfe_dsp_fir_host_buffer": (i32, [vp, C.POINTER(fp), C.POINTER(i32)]),
    "sfe_dsp_fir_process_block": (i32, [vp]),
    "sfe_dsp_fir_process_stream": (i32, [vp, vp, vp, sz, sz, sz, vp]),
    "sfe_dsp_fir_process_host": (i32, [vp, vp, vp, sz]),
    "sfe_dsp_fir_set_algo": (i32, [vp, i32]),
    "sfe_dsp_fir_set_zero_copy_max": (i32, [vp, sz]),
    "sfe_dsp_fir_set_variant": (i32, [vp, i32]),
    "sfe_dsp_fir_get_variant": (i32, [vp, C.POINTER(i32), C.POINTER(i32), fp]),
    "sfe_dsp_fir_forget_calibrations": (i32, []),
    "sfe_dsp_fir_calibrate": (i32, [vp, vp, vp, sz, sz, sz, vp, C.POINTER(i32)]),
    "sfe_dsp_rs_set_algo": (i32, [vp, i32]),
    "sfe_dsp_fir_pipe_create": (i32, [vp, sz, C.POINTER(vp)]),
    "sfe_dsp_rs_pipe_create": (i32, [vp, sz, f32, C.POINTER(vp)]),
    "sfe_dsp_pipe_push": (i32, [vp, vp, sz, C.POINTER(sz)]),
    "sfe_dsp_pipe_pull": (i32, [vp, vp, sz, i32, C.POINTER(sz)]),
    "sfe_dsp_pipe_pending": (i32, [vp, C.POINTER(sz)]),
    "sfe_dsp_pipe_acquire": (i32, [vp, C.POINTER(vp), C.POINTER(sz)]),
    "sfe_dsp_pipe_commit": (i32, [vp, sz]),
    "sfe_dsp_pipe_peek": (i32, [vp, C.POINTER(vp), C.POINTER(sz), i32]),
    "sfe_dsp_pipe_release": (i32, [vp, sz]),
    "sfe_dsp_pipe_destroy": (i32, [vp]),
    "sfe_dsp_fir_load_history": (i32, [vp, vp, sz, sz, vp]),
    "sfe_dsp_rs_load_history": (i32, [vp, vp, sz, sz, vp]),
    "sfe_dsp_rs_seek": (i32, [vp, C.c_uint64, f32]),
    "sfe_dsp_rs_plan_seek": (i32, [C.POINTER(TimeState), i32, C.c_uint64, f32]),
    "sfe_dsp_rs_get_state": (i32, [vp, C.POINTER(TimeState)]),
    "sfe_dsp_rs_set_state": (i32, [vp, C.POINTER(TimeState)]),
    "sfe_dsp_fir_set_input_format": (i32, [vp, i32]),
    "sfe_dsp_fir_set_output_format": (i32, [vp, i32]),
    "sfe_dsp_rs_set_input_format": (i32, [vp, i32]),
    "sfe_dsp_fir_reset": (i32, [vp]),
    "sfe_dsp_fir_destroy": (i32, [vp]),
    "sfe_dsp_rs_create": (i32, [vp, i32, i32, i32, i32, i32, i32, i32, C.POINTER(vp)]),
    "sfe_dsp_rs_process": (i32, [vp, vp, i32, vp, i32, f32, C.POINTER(i32)]),
    "sfe_dsp_rs_process_stream": (i32, [vp, vp, sz, sz, vp, sz, sz, f32, C.POINTER(sz), vp]),
    "sfe_dsp_rs_set_exact": (i32, [vp, i32]),
    "sfe_dsp_rs_reset": (i32, [vp]),
    "sfe_dsp_rs_destroy": (i32, [vp]),
    "sfe_dsp_rs_plan": (i32, [C.POINTER(TimeState), i32, i32, i32, f32, vp, vp, i32, C.POINTER(i32)]),
    "sfe_dsp_fir_group_create": (i32, [vp, i32, i32, i32, i32, i32, C.POINTER(i32), i32, C.POINTER(vp)]),
    "sfe_dsp_fir_group_shards": (i32, [vp, C.POINTER(i32)]),
    "sfe_dsp_fir_group_shard": (i32, [vp, i32, C.POINTER(i32), C.POINTER(i32), C.POINTER(i32), C.POINTER(vp), C.POINTER(vp)]),
    "sfe_dsp_fir_group_process_stream": (i32, [vp, C.POINTER(vp), C.POINTER(vp), sz, sz, sz]),
    "sfe_dsp_fir_group_sync": (i32, [vp]),
    "sfe_dsp_fir_group_reset": (i32, [vp]),
    "sfe_dsp_fir_group_destroy": (i32, [vp]),
    "sfe_dsp_rs_group_create": (i32, [vp, i32, i32, i32, i32, i32, C.POINTER(i32), i32, i32, C.POINTER(vp)]),
    "sfe_dsp_rs_group_shards": (i32, [vp, C.POINTER(i32)]),
    "sfe_dsp_rs_group_shard": (i32, [vp, i32, C.POINTER(i32), C.POINTER(i32), C.POINTER(i32), C.POINTER(vp), C.POINTER(vp)]),
    "sfe_dsp_rs_group_process_stream": (i32, [vp, C.POINTER(vp), sz, sz, C.POINTER(vp), sz, sz, f32, C.POINTER(sz)]),
    "sfe_dsp_rs_group_sync": (i32, [vp]),
    "sfe_dsp_rs_group_reset": (i32, [vp]),
    "sfe_dsp_rs_group_destroy": (i32, [vp]),
    "sfe_dsp_rx_u8_to_f32": (i32, [vp, vp, sz, vp]),
    "sfe_dsp_tx_f32_to_10bit": (i32, [vp, vp, sz, vp]),
    "sfe_dsp_chan_plan": (i32, [i32, i32, i32, C.POINTER(i32), C.POINTER(i32)]),
    "sfe_dsp_chan_create": (i32, [vp, i32, i32, i32, i32, i32, C.POINTER(vp)]),
    "sfe_dsp_chan_set_input_format": (i32, [vp, i32]),
    "sfe_dsp_chan_process_stream": (i32, [vp, vp, sz, sz, vp, sz, C.POINTER(sz), vp]),
    "sfe_dsp_chan_reset": (i32, [vp]),
    "sfe_dsp_chan_destroy": (i32, [vp]),
    "sfe_dsp_combine_plan": (i32, [i32, i32, i32, C.POINTER(i32), C.POINTER(i32)]),
    "sfe_dsp_combine_create": (i32, [vp, i32, i32, i32, i32, i32, C.POINTER(vp)]),
    "sfe_dsp_combine_set_output_format": (i32, [vp, i32]),
    "sfe_dsp_combine_process_stream": (i32, [vp, vp, sz, sz, vp, sz, C.POINTER(sz), vp]),
    "sfe_dsp_combine_reset": (i32, [vp]),
    "sfe_dsp_combine_destroy": (i32, [vp]),
    "sfe_dsp_ddc_plan": (i32, [i32, i32, i32, C.POINTER(C.c_double), C.POINTER(i32), C.POINTER(i32), C.POINTER(C.c_uint32)]),
    "sfe_dsp_ddc_create": (i32, [vp, i32, i32, i32, C.POINTER(C.c_double), i32, i32, i32, C.POINTER(vp)]),
    "sfe_dsp_ddc_set_input_format": (i32, [vp, i32]),
    "sfe_dsp_ddc_set_freqs": (i32, [vp, C.POINTER(C.c_double)]),
    "sfe_dsp_ddc_process_stream": (i32, [vp, vp, sz, sz, vp, sz, C.POINTER(sz), vp]),
    "sfe_dsp_ddc_reset": (i32, [vp]),
    "sfe_dsp_ddc_destroy": (i32, [vp]),
    "sfe_dsp_psd_plan": (i32, [i32, i32, i32, C.POINTER(i32), C.POINTER(i32)]),
    "sfe_dsp_psd_create": (i32, [vp, i32, i32, i32, f32, i32, i32, C.POINTER(vp)]),
    "sfe_dsp_psd_set_input_format": (i32, [vp, i32]),
    "sfe_dsp_psd_process_stream": (i32, [vp, vp, sz, sz, vp, sz, C.POINTER(sz), vp]),
    "sfe_dsp_psd_reset": (i32, [vp]),
    "sfe_dsp_psd_destroy": (i32, [vp]),
    "sfe_dsp_corr_plan": (i32, [i32, i32, i32, C.POINTER(i32), C.POINTER(i32)]),
    "sfe_dsp_corr_create": (i32, [vp, i32, i32, i32, f32, i32, i32, C.POINTER(vp)]),
    "sfe_dsp_corr_set_input_format": (i32, [vp, i32]),
    "sfe_dsp_corr_process_stream": (i32, [vp, vp, sz, sz, vp, vp, sz, vp, sz, C.POINTER(sz), vp]),
    "sfe_dsp_corr_reset": (i32, [vp]),
    "sfe_dsp_corr_destroy": (i32, [vp]),
    "sfe_dsp_iir_plan": (i32, [C.POINTER(C.c_double), i32, C.POINTER(i32), C.POINTER(i32)]),
    "sfe_dsp_iir_create": (i32, [C.POINTER(C.c_double), i32, i32, i32, i32, C.POINTER(vp)]),
    "sfe_dsp_iir_set_input_format": (i32, [vp, i32]),
    "sfe_dsp_iir_process_stream": (i32, [vp, vp, sz, sz, vp, sz, C.POINTER(sz), vp]),
    "sfe_dsp_iir_reset": (i32, [vp]),
    "sfe_dsp_iir_destroy": (i32, [vp]),
    "sfe_dsp_beam_plan": (i32, [i32, i32, i32, fp, fp, fp]),
    "sfe_dsp_beam_create": (i32, [fp, fp, i32, i32, i32, i32, C.POINTER(vp)]),
    "sfe_dsp_beam_set_input_format": (i32, [vp, i32]),
    "sfe_dsp_beam_set_weights": (i32, [vp, fp, fp]),
    "sfe_dsp_beam_process_stream": (i32, [vp, vp, sz, sz, vp, sz, C.POINTER(sz), vp]),
    "sfe_dsp_beam_destroy": (i32, [vp]),
    "sfe_dsp_cov_plan": (i32, [i32, i32, i32, C.POINTER(i32), C.POINTER(i32)]),
    "sfe_dsp_cov_create": (i32, [i32, i32, i32, f32, i32, C.POINTER(vp)]),
    "sfe_dsp_cov_set_input_format": (i32, [vp, i32]),
    "sfe_dsp_cov_process_stream": (i32, [vp, vp, sz, sz, vp, sz, C.POINTER(sz), vp]),
    "sfe_dsp_cov_reset": (i32, [vp]),
    "sfe_dsp_cov_destroy": (i32, [vp]),
    "sfe_dsp_mvdr_plan": (i32, [i32, i32, i32, fp, i32, f32, f32, fp, fp, fp, C.POINTER(i32)]),
    "sfe_dsp_mvdr_create": (i32, [fp, i32, i32, i32, i32, f32, f32, i32, C.POINTER(vp)]),
    "sfe_dsp_mvdr_set_steering": (i32, [vp, fp]),
    "sfe_dsp_mvdr_set_loading": (i32, [vp, f32, f32]),
    "sfe_dsp_mvdr_process_stream": (i32, [vp, vp, sz, sz, vp, sz, vp, sz, vp, sz, C.POINTER(sz), vp]),
    "sfe_dsp_mvdr_load_beam": (i32, [vp, vp, vp]),
    "sfe_dsp_mvdr_destroy": (i32, [vp]),
    "sfe_dsp_eig_plan": (i32, [i32, i32, i32, i32, fp, i32, i32, fp, fp, fp, fp, C.POINTER(i32)]),
    "sfe_dsp_eig_create": (i32, [fp, i32, i32, i32, i32, i32, i32, i32, C.POINTER(vp)]),
    "sfe_dsp_eig_set_steering": (i32, [vp, fp]),
    "sfe_dsp_eig_set_signal_dim": (i32, [vp, i32]),
    "sfe_dsp_eig_process_stream": (i32, [vp, vp, sz, sz, vp, sz, vp, sz, vp, sz, vp, sz, C.POINTER(sz), vp]),
    "sfe_dsp_eig_destroy": (i32, [vp]),
    "sfe_dsp_burst_plan": (i32, [fp, i32, i32, i32, i32, i32, f32, fp, sz, C.POINTER(C.c_uint32), fp, sz, C.c_int64, C.c_int64, fp, fp, fp,
                                 C.POINTER(i32)]),
    "sfe_dsp_burst_create": (i32, [fp, i32, i32, i32, i32, i32, f32, i32, i32, C.POINTER(vp)]),
    "sfe_dsp_burst_set_input_format": (i32, [vp, i32]),
    "sfe_dsp_burst_set_gate": (i32, [vp, f32]),
    "sfe_dsp_burst_process_stream": (i32, [vp, vp, sz, sz, vp, sz, vp, sz, sz, C.c_int64, C.c_int64, vp, sz, vp, vp, sz, C.POINTER(sz), vp]),
    "sfe_dsp_burst_destroy": (i32, [vp]),
    "sfe_dsp_vit_encode": (i32, [i32, i32, C.POINTER(C.c_uint32), C.POINTER(C.c_uint8), i32, i32, C.POINTER(C.c_uint8), sz, C.POINTER(C.c_uint8),
                                 C.POINTER(sz)]),
    "sfe_dsp_vit_footprint": (i32, [i32, i32, i32, i32, C.POINTER(sz), C.POINTER(i32), C.POINTER(i32)]),
    "sfe_dsp_vit_plan": (i32, [i32, i32, C.POINTER(C.c_uint32), C.POINTER(C.c_uint8), i32, i32, i32, i32, i32, fp, sz, C.POINTER(i32), sz,
                               C.POINTER(C.c_uint8), sz, C.POINTER(C.c_uint32), C.POINTER(i32), C.POINTER(sz)]),
    "sfe_dsp_vit_create": (i32, [i32, i32, C.POINTER(C.c_uint32), C.POINTER(C.c_uint8), i32, i32, i32, i32, i32, i32, C.POINTER(vp)]),
    "sfe_dsp_vit_process_stream": (i32, [vp, vp, sz, vp, sz, vp, sz, vp, vp, C.POINTER(sz), vp]),
    "sfe_dsp_vit_destroy": (i32, [vp]),
    "sfe_dsp_mod_footprint": (i32, [C.POINTER(i32), C.POINTER(sz)]),
    "sfe_dsp_mod_plan": (i32, [i32, i32, C.POINTER(C.c_uint32), C.POINTER(C.c_uint8), i32, i32, i32, i32, fp, i32, i32, fp, i32, f32, i32,
                               C.POINTER(C.c_uint8), sz, sz, C.c_int64, C.c_int64, sz, vp, C.POINTER(i32), C.POINTER(i32), C.POINTER(sz)]),
    "sfe_dsp_mod_create": (i32, [i32, i32, C.POINTER(C.c_uint32), C.POINTER(C.c_uint8), i32, i32, i32, i32, fp, i32, i32, fp, i32, f32, i32, i32,
                                 C.POINTER(vp)]),
    "sfe_dsp_mod_process_stream": (i32, [vp, vp, sz, sz, C.c_int64, C.c_int64, vp, sz, C.POINTER(sz), vp]),
    "sfe_dsp_mod_destroy": (i32, [vp]),
    "sfe_dsp_polar_plan": (i32, [i32, f32, i32, vp, sz, fp, fp]),
    "sfe_dsp_polar_create": (i32, [i32, f32, i32, i32, C.POINTER(vp)]),
    "sfe_dsp_polar_set_input_format": (i32, [vp, i32]),
    "sfe_dsp_polar_process_stream": (i32, [vp, vp, sz, sz, vp, sz, C.POINTER(sz), vp]),
    "sfe_dsp_polar_reset": (i32, [vp]),
    "sfe_dsp_polar_destroy": (i32, [vp]),
    "sfe_dsp_occ_plan": (i32, [i32, i32, f32, f32, i32, i32, i32, i32, fp, sz, vp, vp, vp]),
    "sfe_dsp_occ_create": (i32, [i32, i32, f32, f32, i32, i32, i32, i32, i32, C.POINTER(vp)]),
    "sfe_dsp_occ_process_stream": (i32, [vp, vp, sz, sz, sz, vp, vp, vp, sz, C.POINTER(sz), vp]),
    "sfe_dsp_occ_destroy": (i32, [vp]),
    "sfe_dsp_reed_plan": (i32, [i32, i32, i32, i32, i32, i32, vp, i32, vp, sz, vp, sz, vp, sz, vp, vp, C.POINTER(i32), C.POINTER(i32)]),
    "sfe_dsp_reed_create": (i32, [i32, i32, i32, i32, i32, i32, vp, i32, C.POINTER(vp)]),
    "sfe_dsp_reed_encode_stream": (i32, [vp, vp, sz, sz, vp, sz, C.POINTER(sz), vp]),
    "sfe_dsp_reed_process_stream": (i32, [vp, vp, sz, vp, sz, vp, sz, vp, vp, C.POINTER(sz), vp]),
    "sfe_dsp_reed_destroy": (i32, [vp]),
    "sfe_dsp_ldpc_footprint": (i32, [i32, i32, i32, vp, C.POINTER(sz), C.POINTER(i32)]),
    "sfe_dsp_ldpc_plan": (i32, [i32, i32, i32, vp, f32, i32, i32, i32, i32, i32, i32, vp, sz, vp, sz, vp, sz, vp, vp, C.POINTER(i32), C.POINTER(i32),
                                C.POINTER(i32)]),
    "sfe_dsp_ldpc_create": (i32, [i32, i32, i32, vp, f32, i32, i32, i32, i32, i32, i32, C.POINTER(vp)]),
    "sfe_dsp_ldpc_process_stream": (i32, [vp, vp, sz, vp, sz, vp, sz, vp, vp, C.POINTER(sz), vp]),
    "sfe_dsp_ldpc_encode_stream": (i32, [vp, vp, sz, sz, vp, sz, C.POINTER(sz), vp]),
    "sfe_dsp_ldpc_destroy": (i32, [vp]),
    "sfe_dsp_ofdm_plan": (i32, [i32, i32, i32, i32, i32, vp, fp, fp, vp, i32, i32, i32, f32, fp, sz, C.POINTER(C.c_uint32), fp, sz, C.c_int64,
                                C.c_int64, fp, fp, fp, C.POINTER(i32)]),
    "sfe_dsp_ofdm_create": (i32, [i32, i32, i32, i32, i32, vp, fp, fp, vp, i32, i32, i32, f32, i32, i32, C.POINTER(vp)]),
    "sfe_dsp_ofdm_set_input_format": (i32, [vp, i32]),
    "sfe_dsp_ofdm_process_stream": (i32, [vp, vp, sz, sz, vp, sz, vp, sz, sz, C.c_int64, C.c_int64, vp, sz, vp, vp, vp, sz, C.POINTER(sz), vp]),
    "sfe_dsp_ofdm_destroy": (i32, [vp]),
    "sfe_dsp_ofdmmod_footprint": (i32, [i32, C.POINTER(i32), C.POINTER(i32), C.POINTER(sz)]),
    "sfe_dsp_ofdmmod_plan": (i32, [i32, i32, i32, i32, vp, fp, fp, vp, f32, i32, i32, i32, vp, sz, sz, C.c_int64, C.c_int64, sz, vp,
                                   C.POINTER(i32), C.POINTER(i32), C.POINTER(sz)]),
    "sfe_dsp_ofdmmod_create": (i32, [i32, i32, i32, i32, vp, fp, fp, vp, f32, i32, i32, i32, i32, C.POINTER(vp)]),
    "sfe_dsp_ofdmmod_process_stream": (i32, [vp, vp, sz, sz, C.c_int64, C.c_int64, vp, sz, C.POINTER(sz), vp]),
    "sfe_dsp_ofdmmod_destroy": (i32, [vp]),
    "sfe_dsp_qam_plan": (i32, [i32, f32, f32, sz, vp, i32, i32, vp, i32, vp, sz, vp, sz, sz, vp, sz, C.POINTER(i32), C.POINTER(sz)]),
    "sfe_dsp_qam_create": (i32, [i32, f32, f32, sz, vp, i32, i32, vp, i32, C.POINTER(vp)]),
    "sfe_dsp_qam_map_stream": (i32, [vp, vp, sz, sz, vp, sz, C.POINTER(sz), vp]),
    "sfe_dsp_qam_demap_stream": (i32, [vp, vp, sz, vp, sz, sz, vp, sz, C.POINTER(sz), vp]),
    "sfe_dsp_qam_destroy": (i32, [vp]),
    "sfe_dsp_fsk_plan": (i32, [i32, vp, i32, f32, f32, vp, i32, i32, vp, i32, i32, i32, f32, f32, i32, i32, vp, sz, vp, vp, sz, C.c_int64, C.c_int64,
                               vp, sz, vp, vp, vp, C.POINTER(i32), C.POINTER(i32), vp, C.POINTER(f32)]),
    "sfe_dsp_fsk_create": (i32, [i32, vp, i32, f32, f32, vp, i32, i32, vp, i32, i32, i32, f32, f32, i32, i32, i32, C.POINTER(vp)]),
    "sfe_dsp_fsk_set_input_format": (i32, [vp, i32]),
    "sfe_dsp_fsk_mod_stream": (i32, [vp, vp, sz, sz, C.c_int64, C.c_int64, vp, sz, C.POINTER(sz), vp]),
    "sfe_dsp_fsk_demod_stream": (i32, [vp, vp, sz, sz, vp, sz, vp, sz, sz, C.c_int64, C.c_int64, vp, sz, vp, sz, vp, vp, sz, C.POINTER(sz), vp]),
    "sfe_dsp_fsk_destroy": (i32, [vp]),
    "sfe_dsp_crc_pn_bytes": (i32, [i32, u32, u32, sz, vp]),
    "sfe_dsp_crc_plan": (i32, [i32, u32, u32, i32, u32, i32, u32, u32, i32, i32, vp, sz, vp, sz, vp, sz, vp, vp, C.POINTER(i32)]),
    "sfe_dsp_crc_create": (i32, [i32, u32, u32, i32, u32, i32, u32, u32, i32, i32, C.POINTER(vp)]),
    "sfe_dsp_crc_append_stream": (i32, [vp, vp, sz, sz, vp, sz, C.POINTER(sz), vp]),
    "sfe_dsp_crc_check_stream": (i32, [vp, vp, sz, vp, sz, vp, sz, vp, vp, C.POINTER(sz), vp]),
    "sfe_dsp_crc_destroy": (i32, [vp]),
}

# the diagnostic library only (simplefe_amd/csrc/diag/sfe_dsp_diag.h; scripts/ load it by pointing LIB_PATH at it): bound when present
DIAG_SIGNATURES = {
    "sfe_dsp_probe_pair": (i32, [vp, sz, vp, sz, C.POINTER(C.c_float)]),
    "sfe_dsp_malloc_pair": (i32, [sz, sz, C.c_int, C.POINTER(vp), C.POINTER(vp), C.POINTER(C.c_float), C.POINTER(C.c_float)]),
    "sfe_dsp_malloc_pair_screened": (i32, [sz, sz, C.c_int, C.POINTER(vp), C.POINTER(vp), C.POINTER(C.c_float), C.POINTER(C.c_float)]),
    "sfe_dsp_mem_kind": (i32, [vp, C.POINTER(C.c_int)]),
}

_lib = None


def load():
    """Load the in-tree HIP extension.  Raises if it has not been built."""
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(LIB_PATH):
        raise ImportError(
            f"{LIB_PATH} is missing: build it with `python -m simplefe_amd.build` "
            "(hipcc --offload-arch=gfx950).  There is no CPU fallback.")
    L = C.CDLL(LIB_PATH, mode=C.RTLD_GLOBAL)
    for name, (res, args) in SIGNATURES.items():
        fn = getattr(L, name)          # AttributeError if the .so does not export it
        fn.restype = res
        fn.argtypes = args
    for name, (res, args) in DIAG_SIGNATURES.items():
        fn = getattr(L, name, None)
        if fn is not None:
            fn.restype = res
            fn.argtypes = args
    _lib = L
    return L


class SfeError(RuntimeError):
    def __init__(self, code, msg):
        super().__init__(f"libsfe_dsp error {code}: {msg}")
        self.code = code


def check(rc):
    if rc != SFE_OK:
        raise SfeError(rc, load().sfe_dsp_last_error().decode(errors="replace"))
    return rc
