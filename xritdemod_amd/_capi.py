"""ctypes binding of libxritdemod_amd.so (include/xritdemod_amd.h)."""
import ctypes as C
import os
import subprocess

import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))
_LIB = os.path.join(_HERE, "lib", "libxritdemod_amd.so")

SAMPLE_FLOATIQ, SAMPLE_S16IQ, SAMPLE_S8IQ, SAMPLE_U8IQ = 0, 1, 2, 3


class XritError(RuntimeError):
    def __init__(self, code, text):
        super().__init__(f"xritdemod_amd error {code}: {text}")
        self.code = code


class DemodConfig(C.Structure):
    _fields_ = [("sample_rate", C.c_float), ("decimation", C.c_uint32), ("symbol_rate", C.c_uint32),
                ("rrc_alpha", C.c_float), ("rrc_taps", C.c_int32),
                ("agc_rate", C.c_float), ("agc_reference", C.c_float), ("agc_gain", C.c_float),
                ("agc_max_gain", C.c_float), ("pll_alpha", C.c_float),
                ("clock_mu", C.c_float), ("clock_alpha", C.c_float), ("clock_gain_omega", C.c_float),
                ("clock_omega_limit", C.c_float),
                ("device", C.c_int32), ("costas_chain_len", C.c_int32), ("clock_chain_syms", C.c_int32),
                ("max_passes", C.c_int32), ("strict", C.c_int32), ("clock_min_passes", C.c_int32),
                ("slices", C.c_int32), ("clock_serial", C.c_int32), ("clock_exact", C.c_int32),
                ("clock_exact_window", C.c_int32), ("front_exact", C.c_int32), ("reserved", C.c_int32 * 2)]


class DemodStats(C.Structure):
    _fields_ = [("samples_in", C.c_uint64), ("circuit_samples", C.c_uint64), ("symbols_out", C.c_uint64),
                ("costas_passes", C.c_int32), ("clock_passes", C.c_int32),
                ("costas_unconverged", C.c_uint32), ("clock_unconverged", C.c_uint32),
                ("costas_max_residual", C.c_float), ("clock_max_residual", C.c_float),
                ("agc_serial_fallback", C.c_int32), ("clock_open_large", C.c_uint32), ("costas_serial_walk", C.c_int32),
                ("clock_relay_passes", C.c_int32), ("clock_relay_closed", C.c_int32), ("clock_relay_segments", C.c_int32)]


class SynthParams(C.Structure):
    _fields_ = [("fs_in", C.c_double), ("symbol_rate", C.c_double), ("alpha", C.c_double),
                ("amplitude", C.c_double), ("carrier_hz", C.c_double), ("phase0", C.c_double),
                ("timing_offset", C.c_double), ("clock_ppm", C.c_double), ("esn0_db", C.c_double),
                ("seed", C.c_uint64)]


# every symbol include/xritdemod_amd.h declares: (restype, argtypes)
_vp, _sz = C.c_void_p, C.c_size_t
_SIGNATURES = {
    "xrit_last_error": (C.c_char_p, []),
    "xrit_version": (C.c_char_p, []),
    "xrit_device_count": (C.c_int, []),
    "xrit_build_experiments": (C.c_int, []),
    "xrit_lowpass_taps": (C.c_int, [C.c_double] * 4 + [_vp, C.c_int]),
    "xrit_rrc_taps": (C.c_int, [C.c_double] * 4 + [C.c_int, _vp, C.c_int]),
    "xrit_mmse_table": (None, [_vp]),
    "xrit_demod_config_lrit": (None, [C.POINTER(DemodConfig), C.c_float, C.c_uint32]),
    "xrit_demod_config_hrit": (None, [C.POINTER(DemodConfig), C.c_float, C.c_uint32]),
    "xrit_demod_create": (C.c_int, [C.POINTER(DemodConfig), C.POINTER(_vp)]),
    "xrit_demod_destroy": (None, [_vp]),
    "xrit_demod_process": (C.c_int, [_vp, _vp, _sz, C.c_int, _vp, _sz, C.POINTER(_sz)]),
    "xrit_demod_process_device": (C.c_int, [_vp, _vp, _sz, C.c_int, _vp, _sz, C.POINTER(_sz), _vp]),
    "xrit_demod_prefetch_device": (C.c_int, [_vp, _vp, _sz, C.c_int, _vp]),
    "xrit_demod_reset": (C.c_int, [_vp, _vp]),
    "xrit_demod_stream": (_vp, [_vp]),
    "xrit_demod_sps": (C.c_float, [_vp]),
    "xrit_demod_decimator_ntaps": (C.c_int, [_vp]),
    "xrit_demod_keep_stages": (C.c_int, [_vp, C.c_int]),
    "xrit_demod_read_stage": (C.c_int, [_vp, C.c_int, _vp, _sz, C.POINTER(_sz)]),
    "xrit_demod_get_stats": (C.c_int, [_vp, C.POINTER(DemodStats)]),
    "xrit_demod_profile": (C.c_int, [_vp, C.c_int]),
    "xrit_demod_profile_read": (C.c_int, [_vp, C.POINTER(C.c_char_p), C.POINTER(C.c_float), C.POINTER(C.c_int), C.c_int]),
    "xrit_group_restart": (C.c_int, [_vp]),
    "xrit_demod_prepare_flipped": (C.c_int, [_vp, _vp]),
    "xrit_demod_flip_costas_phase": (C.c_int, [_vp, _vp]),
    "xrit_demod_front_exact_for": (C.c_int, [_vp, _sz]),
    "xrit_demod_clock_carry_bytes": (_sz, []),
    "xrit_demod_export_clock_carry": (C.c_int, [_vp, C.c_int, _vp, _vp]),
    "xrit_demod_redo_clock_from": (C.c_int, [_vp, _vp, _vp, _sz, C.POINTER(_sz), _vp]),
    "xrit_demod_last_clock_exact": (C.c_int, [_vp]),
    "xrit_demod_prefetch_depth": (C.c_int, [_vp, _sz]),
    "xrit_demod_redo_clock_flipped": (C.c_int, [_vp, _vp, _sz, C.POINTER(_sz), _vp]),
    "xrit_demod_profile_samples": (C.c_int, [_vp, C.c_char_p, C.POINTER(C.c_float), C.c_int]),
    "xrit_quantize_i8_device": (C.c_int, [_vp, _vp, _sz, C.c_int, _vp]),
    "xrit_quantize_i8": (C.c_int, [_vp, _vp, _vp, _sz]),
    "xrit_sync_correlate_device": (C.c_int, [_vp, _sz, _vp, C.c_int, C.c_uint32, _vp, C.c_int, _vp]),
    "xrit_sync_correlate": (C.c_int, [_vp, _sz, _vp, C.c_int, C.c_uint32, _vp, C.c_int]),
    "xrit_sync_fix_frames_device": (C.c_int, [_vp, _sz, _vp, C.c_uint32, C.c_uint32, _vp, _vp, C.c_int, _vp]),
    "xrit_sync_fix_frames": (C.c_int, [_vp, _sz, _vp, C.c_uint32, C.c_uint32, _vp, _vp, C.c_int]),
    "xrit_framer_create": (C.c_int, [C.POINTER(_vp), C.c_int, C.c_int]),
    "xrit_framer_destroy": (C.c_int, [_vp]),
    "xrit_framer_set_frame": (C.c_int, [_vp, C.c_uint32, C.c_uint32]),
    "xrit_framer_set_segment": (C.c_int, [_vp, C.c_uint32]),
    "xrit_framer_reset": (C.c_int, [_vp]),
    "xrit_framer_rows": (_sz, [_vp, _sz]),
    "xrit_framer_push_device": (C.c_int, [_vp, _vp, _sz, _vp, _vp, _vp, _vp, _vp, _vp]),
    "xrit_framer_push": (C.c_int, [_vp, _vp, _sz, _vp, _vp, _vp, _vp]),
    "xrit_framer_stats": (C.c_int, [_vp, _vp]),
    "xrit_lock_create": (C.c_int, [C.POINTER(_vp), C.c_int, C.c_int]),
    "xrit_lock_destroy": (C.c_int, [_vp]),
    "xrit_lock_reset": (C.c_int, [_vp]),
    "xrit_lock_set_flywheel": (C.c_int, [_vp, C.c_uint32]),
    "xrit_lock_set_segment": (C.c_int, [_vp, C.c_uint32]),
    "xrit_lock_set_windows": (C.c_int, [_vp, C.c_uint32]),
    "xrit_lock_rows": (_sz, [_vp, _sz]),
    "xrit_lock_push_device": (C.c_int, [_vp, _vp, _sz] + [_vp] * 10),
    "xrit_lock_push": (C.c_int, [_vp, _vp, _sz] + [_vp] * 8),
    "xrit_lock_stats": (C.c_int, [_vp, _vp]),
    "xrit_decoder_create": (C.c_int, [C.POINTER(_vp), C.c_int, C.c_int]),
    "xrit_decoder_destroy": (C.c_int, [_vp]),
    "xrit_decoder_reset": (C.c_int, [_vp]),
    "xrit_decoder_set_windows": (C.c_int, [_vp, C.c_uint32]),
    "xrit_decoder_decode_device": (C.c_int, [_vp, _vp, _vp, _sz, _vp, _vp, _vp, _vp]),
    "xrit_decoder_decode": (C.c_int, [_vp, _vp, _vp, _sz, _vp, _vp, _vp]),
    "xrit_demux_create": (C.c_int, [C.POINTER(_vp), C.c_int]),
    "xrit_demux_destroy": (C.c_int, [_vp]),
    "xrit_demux_reset": (C.c_int, [_vp]),
    "xrit_demux_process_device": (C.c_int, [_vp, _vp, _vp, _vp, _vp, _sz, _vp, _vp, _vp, _vp]),
    "xrit_demux_process": (C.c_int, [_vp, _vp, _vp, _vp, _vp, _sz, _vp, _vp, _vp]),
    "xrit_demux_stats": (C.c_int, [_vp, _vp]),
    "xrit_demux_expand": (C.c_int, [_vp, _vp, _sz, _vp]),
    "xrit_packets_create": (C.c_int, [C.POINTER(_vp), C.c_int]),
    "xrit_packets_destroy": (C.c_int, [_vp]),
    "xrit_packets_reset": (C.c_int, [_vp]),
    "xrit_packets_process_device": (C.c_int, [_vp, _vp, _vp, _sz, _vp, _sz, _vp, _sz, _vp, _vp, _vp]),
    "xrit_packets_process": (C.c_int, [_vp, _vp, _vp, _vp, _sz, _vp, _sz, _vp, _vp]),
    "xrit_packets_stats": (C.c_int, [_vp, _vp]),
    "xrit_files_create": (C.c_int, [C.POINTER(_vp), C.c_int]),
    "xrit_files_destroy": (C.c_int, [_vp]),
    "xrit_files_reset": (C.c_int, [_vp]),
    "xrit_files_process_device": (C.c_int, [_vp, _vp, _sz, _vp, _vp, _sz, _vp, _sz, _vp, _sz, _vp, _sz, _vp, _vp]),
    "xrit_files_process": (C.c_int, [_vp, _vp, _sz, _vp, _vp, _vp, _sz, _vp, _sz, _vp, _sz, _vp]),
    "xrit_files_stats": (C.c_int, [_vp, _vp]),
    "xrit_files_key": (C.c_int, [_vp, C.c_uint, C.c_uint, _vp]),
    "xrit_rice_decode_device": (C.c_int, [_vp, _sz, _vp, _sz, _sz, C.c_int, C.c_int, C.c_int, _vp, _vp, C.c_int, _vp]),
    "xrit_rice_form": (C.c_int, [C.c_int]),
    "xrit_rice_decode": (C.c_int, [_vp, _sz, _vp, _sz, _sz, C.c_int, C.c_int, C.c_int, _vp, _vp, C.c_int]),
    "xrit_images_create": (C.c_int, [C.POINTER(_vp), C.c_int]),
    "xrit_images_destroy": (C.c_int, [_vp]),
    "xrit_images_reset": (C.c_int, [_vp]),
    "xrit_images_process_device": (C.c_int, [_vp, _vp, _sz, _vp, _sz, _vp, _sz, _vp, _vp, _sz, _vp, _sz, _vp, _vp, _vp]),
    "xrit_images_process": (C.c_int, [_vp, _vp, _sz, _vp, _sz, _vp, _sz, _vp, _vp, _sz, _vp, _sz, _vp, _vp]),
    "xrit_images_stats": (C.c_int, [_vp, _vp]),
    "xrit_images_key": (C.c_int, [_vp, C.c_uint, C.c_uint, _vp]),
    "xrit_canvas_create": (C.c_int, [C.POINTER(_vp), C.c_int, C.c_uint, _sz]),
    "xrit_canvas_destroy": (C.c_int, [_vp]),
    "xrit_canvas_reset": (C.c_int, [_vp]),
    "xrit_canvas_process_device": (C.c_int, [_vp, _vp, _sz, _vp, _sz, _vp, _sz, _vp, _vp, _sz, _vp, _sz, _vp, _vp, _vp, _vp, _vp, _vp]),
    "xrit_canvas_process": (C.c_int, [_vp, _vp, _sz, _vp, _sz, _vp, _sz, _vp, _vp, _sz, _vp, _sz, _vp, _vp, _vp, _vp, _vp]),
    "xrit_canvas_read_device": (C.c_int, [_vp, C.c_uint, _vp, _sz, _vp]),
    "xrit_canvas_read": (C.c_int, [_vp, C.c_uint, _vp, _sz, _vp]),
    "xrit_canvas_segments": (C.c_int, [_vp, C.c_uint, _vp]),
    "xrit_canvas_key": (C.c_int, [_vp, C.c_uint, C.c_uint, _vp]),
    "xrit_canvas_stats": (C.c_int, [_vp, _vp]),
    "xrit_canvas_release": (C.c_int, [_vp, C.c_uint]),
    "xrit_canvas_pixels_device": (C.c_int, [_vp, C.c_uint, C.POINTER(_vp)]),
    "xrit_product_create": (C.c_int, [C.POINTER(_vp), C.c_int]),
    "xrit_product_destroy": (C.c_int, [_vp]),
    "xrit_product_reset": (C.c_int, [_vp]),
    "xrit_product_process_device": (C.c_int, [_vp] * 10),
    "xrit_product_process": (C.c_int, [_vp] * 9),
    "xrit_product_process_resident": (C.c_int, [_vp] * 9),
    "xrit_product_outputs_device": (C.c_int, [_vp, C.POINTER(_vp), C.POINTER(_vp)]),
    "xrit_product_composite_device": (C.c_int, [_vp, _vp, C.c_uint32, _vp, C.c_uint32, C.c_uint32, C.c_uint32, _vp, _vp, _vp]),
    "xrit_product_composite": (C.c_int, [_vp, _vp, C.c_uint32, _vp, C.c_uint32, C.c_uint32, C.c_uint32, _vp, _vp]),
    "xrit_geo_create": (C.c_int, [C.POINTER(_vp), C.c_int]),
    "xrit_geo_destroy": (C.c_int, [_vp]),
    "xrit_geo_reset": (C.c_int, [_vp]),
    "xrit_geo_grid_tables": (C.c_int, [_vp, C.c_double, _vp, _vp, _vp, _vp]),
    "xrit_geo_set_grid": (C.c_int, [_vp, _vp, C.c_double]),
    "xrit_geo_set_tables": (C.c_int, [_vp, C.c_uint32, C.c_uint32, _vp, _vp, _vp, _vp]),
    "xrit_geo_tables": (C.c_int, [_vp] * 7),
    "xrit_geo_map_device": (C.c_int, [_vp] * 4),
    "xrit_geo_resample_device": (C.c_int, [_vp, _vp, _vp, C.c_uint32, _vp, C.c_uint32, _vp, _vp]),
    "xrit_geo_project_device": (C.c_int, [_vp, _vp, _vp, C.c_uint32, _vp, C.c_uint32, _vp, _vp]),
    "xrit_geo_project": (C.c_int, [_vp, _vp, _vp, C.c_uint32, _vp, C.c_uint32, _vp]),
    "xrit_geo_project_resident": (C.c_int, [_vp, _vp, _vp, C.c_uint32, _vp, C.c_uint32, _vp]),
    "xrit_geo_parse_navigation": (C.c_int, [_vp, C.c_size_t, _vp]),
    "xrit_geo_pixel_to_lonlat": (C.c_int, [_vp, C.c_double, C.c_double, _vp, _vp]),
    "xrit_overlay_create": (C.c_int, [C.POINTER(_vp), C.c_int]),
    "xrit_overlay_destroy": (C.c_int, [_vp]),
    "xrit_overlay_reset": (C.c_int, [_vp]),
    "xrit_overlay_set_form": (C.c_int, [_vp, C.c_uint32]),
    "xrit_overlay_map_device": (C.c_int, [_vp, _vp, _vp, _sz, _vp, _vp]),
    "xrit_overlay_draw_device": (C.c_int, [_vp, _vp, _sz] + [C.c_uint32] * 3 + [_vp] + [C.c_uint32] * 4 + [_vp, _vp]),
    "xrit_overlay_blend_device": (C.c_int, [_vp, _vp, C.c_uint32, _vp, C.c_uint32, _vp, _vp, C.c_uint32, C.c_uint32, _vp, _vp]),
    "xrit_overlay_map": (C.c_int, [_vp, _vp, _vp, _sz, _vp]),
    "xrit_overlay_draw": (C.c_int, [_vp, _vp, _sz] + [C.c_uint32] * 3 + [_vp] + [C.c_uint32] * 4 + [_vp]),
    "xrit_overlay_blend": (C.c_int, [_vp, _vp, C.c_uint32, _vp, C.c_uint32, _vp, _vp, C.c_uint32, C.c_uint32, _vp]),
    "xrit_overlay_blend_resident": (C.c_int, [_vp, _vp, C.c_uint32, _vp, C.c_uint32, _vp, _vp, C.c_uint32, C.c_uint32, _vp]),
    "xrit_overlay_mask_device": (C.c_int, [_vp, C.POINTER(_vp)]),
    "xrit_overlay_quads": (C.c_int, [_vp, _vp, _sz, C.c_double, _vp]),
    "xrit_overlay_grid_points": (C.c_int, [_vp, _vp, _vp, _sz, _vp]),
    "xrit_overlay_densify": (C.c_int, [_vp, _vp, _sz, C.c_double, _vp, _vp, _sz, C.POINTER(_sz)]),
    "xrit_overlay_graticule": (C.c_int, [C.c_double, C.c_double, _vp, _vp, _sz, C.POINTER(_sz)]),
    "xrit_jpeg_create": (C.c_int, [C.POINTER(_vp), C.c_int]),
    "xrit_jpeg_destroy": (C.c_int, [_vp]),
    "xrit_jpeg_reset": (C.c_int, [_vp]),
    "xrit_jpeg_set_quality": (C.c_int, [_vp, C.c_uint32, C.c_uint32]),
    "xrit_jpeg_set_tables": (C.c_int, [_vp, _vp, C.c_uint32]),
    "xrit_jpeg_header": (C.c_int, [_vp, C.c_uint32, C.c_uint32, C.c_uint32, _vp, _sz, C.POINTER(_sz)]),
    "xrit_jpeg_quality_tables": (C.c_int, [C.c_uint32, _vp]),
    "xrit_jpeg_header_for": (C.c_int, [_vp, C.c_uint32, C.c_uint32, C.c_uint32, C.c_uint32, _vp, _sz, C.POINTER(_sz)]),
    "xrit_jpeg_bound": (C.c_uint64, [C.c_uint32] * 4),
    "xrit_jpeg_encode_device": (C.c_int, [_vp, _vp, C.c_uint32, _vp, _sz, _vp, _vp]),
    "xrit_jpeg_encode": (C.c_int, [_vp, _vp, C.c_uint32, _vp, _sz, _vp]),
    "xrit_jpeg_encode_resident": (C.c_int, [_vp, _vp, C.c_uint32, _vp, _sz, _vp]),
    "xrit_jpegdec_create": (C.c_int, [C.POINTER(_vp), C.c_int]),
    "xrit_jpegdec_destroy": (C.c_int, [_vp]),
    "xrit_jpegdec_reset": (C.c_int, [_vp]),
    "xrit_jpegdec_set_form": (C.c_int, [_vp, C.c_uint32, C.c_uint32]),
    "xrit_jpegdec_header": (C.c_int, [_vp, _sz, _vp]),
    "xrit_jpegdec_decode_device": (C.c_int, [_vp, _vp, _sz, _vp, _sz, _sz, _sz, _vp, _sz, _vp, _vp, _vp]),
    "xrit_jpegdec_decode": (C.c_int, [_vp, _vp, _sz, _vp, _sz, _sz, _vp, _sz, _vp, _vp]),
    "xrit_jpegdec_rounds": (C.c_int, [_vp, C.POINTER(C.c_uint32)]),
    "xrit_acquire_create": (C.c_int, [C.POINTER(_vp), _vp, C.c_int]),
    "xrit_acquire_destroy": (C.c_int, [_vp]),
    "xrit_acquire_reset": (C.c_int, [_vp]),
    "xrit_acquire_set_frequency": (C.c_int, [_vp, C.c_double]),
    "xrit_acquire_estimate_device": (C.c_int, [_vp, _vp, _sz, C.c_int, C.c_int, _vp, _vp]),
    "xrit_acquire_mix_device": (C.c_int, [_vp, _vp, _sz, C.c_int, _vp, _vp]),
    "xrit_acquire_estimate": (C.c_int, [_vp, _vp, _sz, C.c_int, C.c_int, _vp]),
    "xrit_acquire_mix": (C.c_int, [_vp, _vp, _sz, C.c_int, _vp]),
    "xrit_acquire_get_state": (C.c_int, [_vp, _vp]),
    "xrit_monitor_create": (C.c_int, [C.POINTER(_vp), C.c_uint32, C.c_int, C.c_int]),
    "xrit_monitor_destroy": (C.c_int, [_vp]),
    "xrit_monitor_reset": (C.c_int, [_vp]),
    "xrit_monitor_rows": (_sz, [_vp, _sz]),
    "xrit_monitor_push_device": (C.c_int, [_vp, _vp, _sz, _vp, _sz, _vp, _vp]),
    "xrit_monitor_push": (C.c_int, [_vp, _vp, _sz, _vp, _sz, C.POINTER(_sz)]),
    "xrit_monitor_get_state": (C.c_int, [_vp, _vp]),
    "xrit_monitor_derive": (C.c_int, [_vp, C.c_int, _vp]),
    "xrit_fir_create": (C.c_int, [C.c_uint, _vp, C.c_int, C.c_int, C.POINTER(_vp)]),
    "xrit_fir_work": (C.c_int, [_vp, _vp, _vp, _sz]),
    "xrit_fir_set_exact": (C.c_int, [_vp, C.c_int]),
    "xrit_loop_sincosf": (C.c_int, [_vp, _vp, _vp, _sz, C.c_int]),
    "xrit_agc_set_exact": (C.c_int, [_vp, C.c_int]),
    "xrit_agc_exact_stats": (C.c_int, [_vp, C.POINTER(C.c_uint32)]),
    "xrit_costas_set_exact": (C.c_int, [_vp, C.c_int, C.c_int]),
    "xrit_costas_exact_stats": (C.c_int, [_vp, C.POINTER(C.c_uint64), C.POINTER(C.c_uint64), C.POINTER(C.c_uint32), C.POINTER(C.c_uint32),
                                          C.POINTER(C.c_uint64), C.POINTER(C.c_uint64)]),
    "xrit_fir_destroy": (None, [_vp]),
    "xrit_agc_create": (C.c_int, [C.c_float] * 4 + [C.c_int, C.POINTER(_vp)]),
    "xrit_agc_work": (C.c_int, [_vp, _vp, _vp, _sz]),
    "xrit_agc_gain": (C.c_float, [_vp]),
    "xrit_agc_destroy": (None, [_vp]),
    "xrit_costas_create": (C.c_int, [C.c_float, C.c_int, C.c_int, C.POINTER(_vp)]),
    "xrit_costas_work": (C.c_int, [_vp, _vp, _vp, _sz]),
    "xrit_costas_state": (C.c_int, [_vp, C.POINTER(C.c_float), C.POINTER(C.c_float)]),
    "xrit_costas_destroy": (None, [_vp]),
    "xrit_clock_create": (C.c_int, [C.c_float] * 5 + [C.c_int, C.POINTER(_vp)]),
    "xrit_clock_work": (C.c_int, [_vp, _vp, _sz, _vp, _sz, C.POINTER(_sz)]),
    "xrit_clock_set_serial": (C.c_int, [_vp, C.c_int]),
    "xrit_clock_set_exact": (C.c_int, [_vp, C.c_int, C.c_int]),
    "xrit_clock_destroy": (None, [_vp]),
    "xrit_group_unique_id": (C.c_int, [_vp]),
    "xrit_group_create": (C.c_int, [C.POINTER(DemodConfig), C.c_int, C.c_int, _vp, C.POINTER(_vp)]),
    "xrit_group_create_all": (C.c_int, [C.POINTER(DemodConfig), C.POINTER(C.c_int), C.c_int, C.POINTER(_vp)]),
    "xrit_local_fabric_create": (C.c_int, [C.c_int, C.POINTER(_vp)]),
    "xrit_local_fabric_destroy": (None, [_vp]),
    "xrit_group_create_local": (C.c_int, [C.POINTER(DemodConfig), C.c_int, _vp, C.POINTER(_vp)]),
    "xrit_group_destroy": (None, [_vp]),
    "xrit_group_chain": (_vp, [_vp]),
    "xrit_group_rank": (C.c_int, [_vp]),
    "xrit_group_world": (C.c_int, [_vp]),
    "xrit_group_halo_samples": (_sz, [_vp]),
    "xrit_group_counters": (None, [_vp, C.POINTER(C.c_uint64), C.POINTER(C.c_uint64), C.POINTER(C.c_uint64)]),
    "xrit_group_rccl_ranks": (C.c_int, [_vp]),
    "xrit_group_process_slice_device": (C.c_int, [_vp, _vp, _sz, C.c_int, _vp, _sz, C.POINTER(_sz), C.POINTER(C.c_uint64),
                                                  C.POINTER(C.c_int), _vp]),
    "xrit_group_process_slice_host": (C.c_int, [_vp, _vp, _sz, C.c_int, _vp, _sz, C.POINTER(_sz), C.POINTER(C.c_uint64),
                                                C.POINTER(C.c_int)]),
    "xrit_group_allreduce_max": (C.c_int, [_vp, C.POINTER(C.c_double), _vp]),
    "xrit_device_read_bandwidth": (C.c_int, [_vp, _sz, C.c_int, C.c_int, _vp, C.POINTER(C.c_double)]),
    "xrit_rtl_create": (C.c_int, [C.c_float, C.c_int, C.POINTER(_vp)]),
    "xrit_rtl_work": (C.c_int, [_vp, _vp, _sz, _vp]),
    "xrit_rtl_destroy": (None, [_vp]),
    "xrit_synth_defaults": (None, [C.POINTER(SynthParams)]),
    "xrit_synth_generate_device": (C.c_int, [C.POINTER(SynthParams), C.c_uint64, _sz, _vp, C.c_int, _vp]),
}

_lib = None


def lib_path():
    return _LIB


def build(force=False):
    """Compile libxritdemod_amd.so for gfx950 with hipcc (csrc/Makefile)."""
    cmd = ["make", "-C", os.path.join(_HERE, "csrc"), "-j8", "-s"]
    if force:
        cmd.append("-B")
    subprocess.check_call(cmd)
    return _LIB


def lib():
    """Load the HIP library; fails loudly when it has not been built."""
    global _lib
    if _lib is None:
        if not os.path.exists(_LIB):
            raise XritError(-2, f"{_LIB} is missing: run `python -c 'import __graft_entry__ as g; g.build()'` "
                                "(the HIP extension is required; there is no CPU path)")
        L = C.CDLL(_LIB)
        for name, (res, args) in _SIGNATURES.items():
            fn = getattr(L, name)
            fn.restype = res
            fn.argtypes = args
        _lib = L
    return _lib


def _check(rc):
    if rc != 0:
        raise XritError(rc, lib().xrit_last_error().decode("utf-8", "replace"))


def device_count():
    return lib().xrit_device_count()


def build_experiments():
    """True when the library carries the measurement switches (make EXTRA=-DXRIT_EXPERIMENTS)."""
    return bool(lib().xrit_build_experiments())


def version():
    return lib().xrit_version().decode()


def _p(a):
    return a.ctypes.data_as(C.c_void_p)


def _c64(a):
    return np.ascontiguousarray(a, dtype=np.complex64)


class Filters:
    """SatHelper::Filters (demodulator.cpp:443-444)."""

    @staticmethod
    def RRC(gain, sample_rate, symbol_rate, alpha, ntaps):
        t = np.zeros(ntaps | 1, np.float32)
        n = lib().xrit_rrc_taps(gain, sample_rate, symbol_rate, alpha, ntaps, _p(t), len(t))
        assert n == len(t)
        return t

    @staticmethod
    def lowPass(gain, sample_rate, cutoff, transition_width, window="HAMMING", beta=6.76):
        if window != "HAMMING":
            raise ValueError("the reference only uses FFTWindows::HAMMING (demodulator.cpp:444)")
        n = -lib().xrit_lowpass_taps(gain, sample_rate, cutoff, transition_width, None, 0)
        t = np.zeros(n, np.float32)
        assert lib().xrit_lowpass_taps(gain, sample_rate, cutoff, transition_width, _p(t), n) == n
        return t

    @staticmethod
    def mmse_table():
        t = np.zeros((129, 8), np.float32)
        lib().xrit_mmse_table(_p(t))
        return t


def loop_sincosf(x, device=0):
    """The exact Costas loop's sincosf (csrc/exact_sincos.h) on the device: (sin, cos) of an array of float32, |x| < 120."""
    x = np.ascontiguousarray(x, np.float32)
    s, c = np.empty_like(x), np.empty_like(x)
    _check(lib().xrit_loop_sincosf(_p(x), _p(s), _p(c), len(x), device))
    return s, c


class _Handle:
    _destroy = None

    def __init__(self):
        self._h = C.c_void_p()

    def close(self):
        if getattr(self, "_h", None) and self._h.value:
            getattr(lib(), self._destroy)(self._h)
            self._h = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class FirFilter(_Handle):
    """SatHelper::FirFilter(decimation, taps); Work(in, out, nOut)."""
    _destroy = "xrit_fir_destroy"

    def __init__(self, decimation, taps, device=0, exact=False):
        super().__init__()
        taps = np.ascontiguousarray(taps, np.float32)
        self.D = int(decimation)
        _check(lib().xrit_fir_create(self.D, _p(taps), len(taps), device, C.byref(self._h)))
        if exact:       # summed in the CPU chain's order (cfg.front_exact = 2)
            _check(lib().xrit_fir_set_exact(self._h, 1))

    def Work(self, x, n_out):
        x = _c64(x)
        assert len(x) >= n_out * self.D
        out = np.zeros(n_out, np.complex64)
        _check(lib().xrit_fir_work(self._h, _p(x), _p(out), n_out))
        return out


class AGC(_Handle):
    """SatHelper::AGC(rate, reference, gain, maxGain); Work(in, out, n)."""
    _destroy = "xrit_agc_destroy"

    def __init__(self, rate, reference, gain, max_gain, device=0, exact=False):
        super().__init__()
        _check(lib().xrit_agc_create(rate, reference, gain, max_gain, device, C.byref(self._h)))
        if exact:       # the float32 recurrence walked literally (cfg.front_exact = 2)
            _check(lib().xrit_agc_set_exact(self._h, 1))

    def Work(self, x):
        x = _c64(x)
        out = np.zeros(len(x), np.complex64)
        _check(lib().xrit_agc_work(self._h, _p(x), _p(out), len(x)))
        return out

    @property
    def gain(self):
        return lib().xrit_agc_gain(self._h)

    def exact_stats(self):
        c = (C.c_uint32 * 8)()
        _check(lib().xrit_agc_exact_stats(self._h, c))
        return {"joints_open": c[0], "blocks": c[1], "picard_rounds": c[2], "at_round_limit": c[3], "lattice_segments": c[4],
                "lattice_fallbacks": c[5]}


class CostasLoop(_Handle):
    """SatHelper::CostasLoop(loopBw, order); Work(in, out, n)."""
    _destroy = "xrit_costas_destroy"

    def __init__(self, loop_bw, order=2, device=0, exact=False, history=0):
        super().__init__()
        _check(lib().xrit_costas_create(loop_bw, order, device, C.byref(self._h)))
        if exact:       # the output on the serial float32 trajectory (cfg.front_exact = 2)
            _check(lib().xrit_costas_set_exact(self._h, 1, int(history)))

    def exact_stats(self):
        b, r, o, f, sg, fb = C.c_uint64(), C.c_uint64(), C.c_uint32(), C.c_uint32(), C.c_uint64(), C.c_uint64()
        _check(lib().xrit_costas_exact_stats(self._h, C.byref(b), C.byref(r), C.byref(o), C.byref(f), C.byref(sg), C.byref(fb)))
        return {"blocks": b.value, "picard_rounds": r.value, "joints_open_after_batch": o.value, "host_rounds": f.value,
                "lattice_segments": sg.value, "lattice_fallbacks": fb.value}

    def Work(self, x):
        x = _c64(x)
        out = np.zeros(len(x), np.complex64)
        _check(lib().xrit_costas_work(self._h, _p(x), _p(out), len(x)))
        return out

    def state(self):
        ph, fr = C.c_float(), C.c_float()
        _check(lib().xrit_costas_state(self._h, C.byref(ph), C.byref(fr)))
        return ph.value, fr.value


class ClockRecovery(_Handle):
    """SatHelper::ClockRecovery(omega, gainOmega, mu, gainMu, omegaRelativeLimit); Work(in, out, n) -> symbols."""
    _destroy = "xrit_clock_destroy"

    def __init__(self, omega, gain_omega, mu, gain_mu, omega_rel_limit, device=0, serial=False, exact=0, window=0):
        super().__init__()
        _check(lib().xrit_clock_create(omega, gain_omega, mu, gain_mu, omega_rel_limit, device, C.byref(self._h)))
        if serial:
            _check(lib().xrit_clock_set_serial(self._h, 1))
        if exact:
            _check(lib().xrit_clock_set_exact(self._h, int(exact), int(window)))

    def Work(self, x):
        x = _c64(x)
        cap = len(x) + 64
        out = np.zeros(cap, np.complex64)
        n = C.c_size_t(0)
        _check(lib().xrit_clock_work(self._h, _p(x), len(x), _p(out), cap, C.byref(n)))
        return out[:n.value].copy()


class RtlIngest(_Handle):
    """RtlFrontend's byte -> float conversion with its DC tracker (RtlFrontend.cpp:26-28,57,102-116)."""
    _destroy = "xrit_rtl_destroy"

    def __init__(self, sample_rate, device=0):
        super().__init__()
        _check(lib().xrit_rtl_create(sample_rate, device, C.byref(self._h)))

    def Work(self, data):
        d = np.ascontiguousarray(data, np.uint8)
        n = len(d) // 2
        out = np.zeros(n, np.complex64)
        _check(lib().xrit_rtl_work(self._h, _p(d), n, _p(out)))
        return out


class Demodulator(_Handle):
    """The chain of processSamples() (demodulator.cpp:100-168) behind one handle."""
    _destroy = "xrit_demod_destroy"
    STAGES = ("decimator", "agc", "rrc", "costas", "clock")

    @staticmethod
    def config(mode="lrit", sample_rate=1.25e6, decimation=1, device=0, **over):
        c = DemodConfig()
        if mode == "lrit":
            lib().xrit_demod_config_lrit(C.byref(c), sample_rate, decimation)
        elif mode == "hrit":
            lib().xrit_demod_config_hrit(C.byref(c), sample_rate, decimation)
        else:
            raise ValueError(mode)
        c.device = device
        for k, v in over.items():
            setattr(c, k, v)
        return c

    def __init__(self, cfg):
        super().__init__()
        self.cfg = cfg
        _check(lib().xrit_demod_create(C.byref(cfg), C.byref(self._h)))

    @property
    def sps(self):
        return lib().xrit_demod_sps(self._h)

    @property
    def decimator_ntaps(self):
        return lib().xrit_demod_decimator_ntaps(self._h)

    def reset(self, stream=None):
        """Back to the freshly created state (another stream begins); device buffers are kept."""
        _check(lib().xrit_demod_reset(self._h, C.c_void_p(stream) if stream else None))

    def prefetch_depth(self, n):
        """Inputs of n samples that may wait behind the call in progress (xrit_demod_prefetch_depth)."""
        return lib().xrit_demod_prefetch_depth(self._h, n)

    def redo_clock_flipped(self, d_soft_ptr, cap, stream=None):
        """The last call's clock recovery once more on the sign-flipped Costas output (xrit_demod_redo_clock_flipped)."""
        n_out = C.c_size_t(0)
        _check(lib().xrit_demod_redo_clock_flipped(self._h, C.c_void_p(d_soft_ptr), cap, C.byref(n_out),
                                                   C.c_void_p(stream) if stream else None))
        return n_out.value

    def prepare_flipped(self, stream=None):
        _check(lib().xrit_demod_prepare_flipped(self._h, C.c_void_p(stream) if stream else None))

    def flip_costas_phase(self, stream=None):
        """Move the carried Costas phase by pi (a freshly reset chain then pulls into its other lock)."""
        _check(lib().xrit_demod_flip_costas_phase(self._h, C.c_void_p(stream) if stream else None))

    def export_clock_carry(self, d_record_ptr, which=0, stream=None):
        """The clock recovery's carried state into a device record of clock_carry_bytes() bytes."""
        _check(lib().xrit_demod_export_clock_carry(self._h, int(which), C.c_void_p(d_record_ptr), C.c_void_p(stream) if stream else None))

    def redo_clock_from(self, d_record_ptr, d_soft_ptr, cap, stream=None):
        """The last call's clock recovery once more from another handle's carried state; returns the symbol count."""
        n_out = _sz(0)
        _check(lib().xrit_demod_redo_clock_from(self._h, C.c_void_p(d_record_ptr), C.c_void_p(d_soft_ptr), cap, C.byref(n_out),
                                                C.c_void_p(stream) if stream else None))
        return n_out.value

    def last_clock_exact(self):
        return lib().xrit_demod_last_clock_exact(self._h) == 1

    def front_exact_for(self, n):
        """True if a call of n input samples takes the bit-exact front end on this handle."""
        r = lib().xrit_demod_front_exact_for(self._h, int(n))
        _check(r if r < 0 else 0)
        return r == 1

    def keep_stages(self, enable=True):
        _check(lib().xrit_demod_keep_stages(self._h, int(enable)))

    def process(self, samples, sample_type=SAMPLE_FLOATIQ):
        """Host buffers in, host soft symbols out."""
        if sample_type == SAMPLE_FLOATIQ:
            a = _c64(samples)
            n = len(a)
        elif sample_type == SAMPLE_S16IQ:
            a = np.ascontiguousarray(samples, np.int16)
            n = len(a) // 2
        elif sample_type == SAMPLE_U8IQ:
            a = np.ascontiguousarray(samples, np.uint8)
            n = len(a) // 2
        else:
            a = np.ascontiguousarray(samples, np.int8)
            n = len(a) // 2
        cap = n + 64
        out = np.zeros(cap, np.float32)
        n_out = C.c_size_t(0)
        _check(lib().xrit_demod_process(self._h, _p(a), n, sample_type, _p(out), cap, C.byref(n_out)))
        return out[:n_out.value].copy()

    def process_device(self, d_samples_ptr, n, d_soft_ptr, cap, sample_type=SAMPLE_FLOATIQ, stream=None):
        """Device pointers (ints) in and out; returns the symbol count."""
        n_out = C.c_size_t(0)
        _check(lib().xrit_demod_process_device(self._h, C.c_void_p(d_samples_ptr), n, sample_type,
                                               C.c_void_p(d_soft_ptr), cap, C.byref(n_out),
                                               C.c_void_p(stream) if stream else None))
        return n_out.value

    def prefetch_device(self, d_samples_ptr, n, sample_type=SAMPLE_FLOATIQ, stream=None):
        """Start the front end of the NEXT process_device call's input now (it overlaps the loops of the call in between)."""
        _check(lib().xrit_demod_prefetch_device(self._h, C.c_void_p(d_samples_ptr), n, sample_type,
                                                C.c_void_p(stream) if stream else None))

    def stage(self, name):
        idx = self.STAGES.index(name)
        n = C.c_size_t(0)
        _check(lib().xrit_demod_read_stage(self._h, idx, None, 0, C.byref(n)))
        out = np.zeros(n.value, np.complex64)
        if n.value:
            _check(lib().xrit_demod_read_stage(self._h, idx, _p(out), n.value, C.byref(n)))
        return out

    def stats(self):
        s = DemodStats()
        _check(lib().xrit_demod_get_stats(self._h, C.byref(s)))
        return s

    def profile(self, enable=True):
        """True/1: bracket every kernel with HIP events; 2: only the decimating FIR; False/0: off."""
        _check(lib().xrit_demod_profile(self._h, int(enable)))

    def profile_read(self):
        cap = 64
        names = (C.c_char_p * cap)()
        ms = (C.c_float * cap)()
        cnt = (C.c_int * cap)()
        n = lib().xrit_demod_profile_read(self._h, names, ms, cnt, cap)
        return [(names[i].decode(), float(ms[i]), int(cnt[i])) for i in range(n)]

    def profile_samples(self, name, cap=4096):
        """Every bracket of one kernel name since profile(enable), in launch order (ms)."""
        ms = (C.c_float * cap)()
        n = lib().xrit_demod_profile_samples(self._h, name.encode(), ms, cap)
        return [float(ms[i]) for i in range(max(n, 0))]

    def quantize_i8(self, soft):
        soft = np.ascontiguousarray(soft, np.float32)
        out = np.zeros(len(soft), np.int8)
        _check(lib().xrit_quantize_i8(self._h, _p(soft), _p(out), len(soft)))
        return out


def synth_generate_device(params, start, n, d_out_ptr, device=0, stream=None):
    _check(lib().xrit_synth_generate_device(C.byref(params), start, n, C.c_void_p(d_out_ptr), device,
                                            C.c_void_p(stream) if stream else None))


GROUP_ID_BYTES = 128


def group_unique_id():
    """ncclGetUniqueId as bytes: rank 0 makes it, the launcher hands it to every rank."""
    buf = (C.c_char * GROUP_ID_BYTES)()
    _check(lib().xrit_group_unique_id(buf))
    return bytes(buf)


class LocalFabric(_Handle):
    """In-process exchange between the ranks of a Group (threads of one process)."""
    _destroy = "xrit_local_fabric_destroy"

    def __init__(self, world):
        super().__init__()
        self.world = world
        _check(lib().xrit_local_fabric_create(world, C.byref(self._h)))


class Group(_Handle):
    """One capture across the GPUs of a node (xrit_group_*): Group(cfg, rank, world, unique_id) with RCCL, or
    Group(cfg, rank, fabric=LocalFabric(world)) for ranks that are threads of one process."""
    _destroy = "xrit_group_destroy"

    def __init__(self, cfg, rank, world=None, unique_id=None, fabric=None):
        super().__init__()
        self.cfg = cfg
        self._fabric = fabric
        if fabric is not None:
            _check(lib().xrit_group_create_local(C.byref(cfg), rank, fabric._h, C.byref(self._h)))
        else:
            idb = (C.c_char * GROUP_ID_BYTES).from_buffer_copy(unique_id)
            _check(lib().xrit_group_create(C.byref(cfg), rank, world, idb, C.byref(self._h)))

    @property
    def halo_samples(self):
        return lib().xrit_group_halo_samples(self._h)

    def counters(self):
        """(relocks, handovers, joined): slices started a second time from the other Costas lock, slices whose clock recovery
        ran again from the loop state of the rank in front, slices that had met that state inside their halo."""
        a, b, c = C.c_uint64(0), C.c_uint64(0), C.c_uint64(0)
        lib().xrit_group_counters(self._h, C.byref(a), C.byref(b), C.byref(c))
        return int(a.value), int(b.value), int(c.value)

    @property
    def relocks(self):
        return self.counters()[0]

    @property
    def rccl_ranks(self):
        """Ranks of the RCCL communicator behind the group, as ncclCommCount reports them (0: in-process fabric)."""
        return lib().xrit_group_rccl_ranks(self._h)

    @property
    def rank(self):
        return lib().xrit_group_rank(self._h)

    @property
    def world(self):
        return lib().xrit_group_world(self._h)

    def chain_process_device(self, d_samples_ptr, n, d_soft_ptr, cap, sample_type=SAMPLE_FLOATIQ, stream=None):
        """Independent segments: the rank's own chain, no exchange."""
        n_out = C.c_size_t(0)
        _check(lib().xrit_demod_process_device(lib().xrit_group_chain(self._h), C.c_void_p(d_samples_ptr), n, sample_type,
                                               C.c_void_p(d_soft_ptr), cap, C.byref(n_out),
                                               C.c_void_p(stream) if stream else None))
        return n_out.value

    def process_slice_device(self, d_samples_ptr, n, d_soft_ptr, cap, sample_type=SAMPLE_FLOATIQ, stream=None):
        """Collective: (symbol count, offset in the burst's symbol sequence, absolute polarity)."""
        n_out, off, pol = C.c_size_t(0), C.c_uint64(0), C.c_int(1)
        _check(lib().xrit_group_process_slice_device(self._h, C.c_void_p(d_samples_ptr), n, sample_type,
                                                     C.c_void_p(d_soft_ptr), cap, C.byref(n_out), C.byref(off),
                                                     C.byref(pol), C.c_void_p(stream) if stream else None))
        return n_out.value, off.value, pol.value

    def restart(self):
        """The next slice call is a capture's first (rank 0 starts cold, nothing is taken over from the last rank)."""
        _check(lib().xrit_group_restart(self._h))

    def allreduce_max(self, value, stream=None):
        v = C.c_double(value)
        _check(lib().xrit_group_allreduce_max(self._h, C.byref(v), C.c_void_p(stream) if stream else None))
        return v.value


def device_read_bandwidth(d_buf_ptr, nbytes, reps=10, device=0, stream=None):
    """GB/s of a hand-written read-only sweep over a device buffer (measurement helper)."""
    out = C.c_double(0)
    _check(lib().xrit_device_read_bandwidth(C.c_void_p(d_buf_ptr), nbytes, reps, device,
                                            C.c_void_p(stream) if stream else None, C.byref(out)))
    return out.value


def synth_params(**over):
    p = SynthParams()
    lib().xrit_synth_defaults(C.byref(p))
    for k, v in over.items():
        setattr(p, k, v)
    return p


def quantize_i8_device(d_soft_ptr, d_out_ptr, n, device=0, stream=None):
    _check(lib().xrit_quantize_i8_device(C.c_void_p(d_soft_ptr), C.c_void_p(d_out_ptr), n, device,
                                         C.c_void_p(stream) if stream else None))


# ---- decoder front end: frame synchronisation (decoder/src/newdecoder.cpp:21-24,145-151,218-245) ----------------
LRIT_UW0, LRIT_UW2 = 0xfca2b63db00d9794, 0x035d49c24ff2686b
HRIT_UW0, HRIT_UW2 = 0xfc4ef4fd0cc2df89, 0x25010b02f33d2076
CODED_FRAME_SIZE = 16384
MIN_CORRELATION_BITS = 46


def sync_correlate(symbols, words=(LRIT_UW0, LRIT_UW2), frame=CODED_FRAME_SIZE, device=0):
    """SatHelper::Correlator over consecutive windows of `frame` int8 soft symbols: array of (word, position,
    correlation) rows, one per window."""
    d = np.ascontiguousarray(symbols, np.int8)
    w = np.asarray(words, np.uint64)
    nf = len(d) // frame
    hits = np.zeros((nf, 4), np.uint32)
    _check(lib().xrit_sync_correlate(_p(d), len(d), _p(w), len(w), frame, _p(hits), device))
    return hits[:, :3].copy()


def sync_fix_frames(symbols, hits, frame=CODED_FRAME_SIZE, min_correlation=MIN_CORRELATION_BITS, device=0):
    """Frame alignment + phase fix between correlator and Viterbi (newdecoder.cpp:239-270): (frames, valid) --
    frames[f] starts at hits[f]'s position, inverted when the 180-degree word won; valid[f] = 0 (zeros) below the
    acceptance or past the end of the buffer.  hits: rows of (word, position, correlation)."""
    d = np.ascontiguousarray(symbols, np.int8)
    nf = len(d) // frame
    h = np.zeros((nf, 4), np.uint32)
    h[:, :3] = np.asarray(hits, np.uint32)[:nf, :3]
    frames = np.zeros((nf, frame), np.int8)
    valid = np.zeros(nf, np.uint8)
    _check(lib().xrit_sync_fix_frames(_p(d), len(d), _p(h), frame, min_correlation, _p(frames), _p(valid), device))
    return frames, valid


def sync_fix_frames_device(d_symbols_ptr, n, d_hits_ptr, d_frames_ptr, d_valid_ptr, frame=CODED_FRAME_SIZE,
                           min_correlation=MIN_CORRELATION_BITS, device=0, stream=None):
    _check(lib().xrit_sync_fix_frames_device(C.c_void_p(d_symbols_ptr), n, C.c_void_p(d_hits_ptr), frame, min_correlation,
                                             C.c_void_p(d_frames_ptr), C.c_void_p(d_valid_ptr), device,
                                             C.c_void_p(stream) if stream else None))


def sync_correlate_device(d_symbols_ptr, n, d_hits_ptr, words=(LRIT_UW0, LRIT_UW2), frame=CODED_FRAME_SIZE, device=0,
                          stream=None):
    w = np.asarray(words, np.uint64)
    _check(lib().xrit_sync_correlate_device(C.c_void_p(d_symbols_ptr), n, _p(w), len(w), frame, C.c_void_p(d_hits_ptr),
                                            device, C.c_void_p(stream) if stream else None))


# ---- stream frame synchroniser: the decoder's walk over a stream, chunk by chunk (newdecoder.cpp:212-270) -----
# xrit_framer_counters
FRAMER_STATS_DTYPE = np.dtype([(f, np.uint64) for f in ("symbols", "cursor", "rows", "frames", "dropped_chunks", "resyncs", "carry",
                                                        "rewalked_chunks", "adopted_chunks", "calls")])
assert FRAMER_STATS_DTYPE.itemsize == 80
FRAMER_MAX_SYMBOLS = 1 << 30


class FrameSynchroniser(_Handle):
    """The reference decoder's frame synchronisation over a stream of int8 soft symbols that arrives in calls of any
    length: a cursor and the symbols not consumed yet are kept on the device, every chunk of `frame` symbols from the
    cursor on is correlated, a hit moves the cursor behind its frame, a miss by one chunk.  The rows do not depend on how
    the stream is cut into calls.  mode: "lrit" (frames found with the inverted word are inverted) or "hrit"."""
    _destroy = "xrit_framer_destroy"

    def __init__(self, mode="lrit", device=0, frame=None, min_correlation=None, segment=0):
        super().__init__()
        if mode not in ("lrit", "hrit"):
            raise ValueError(f"mode {mode!r}: 'lrit' or 'hrit'")
        self.mode = mode
        _check(lib().xrit_framer_create(C.byref(self._h), 1 if mode == "hrit" else 0, device))
        self.frame = CODED_FRAME_SIZE
        if frame is not None or min_correlation is not None:
            self.set_frame(CODED_FRAME_SIZE if frame is None else frame,
                           MIN_CORRELATION_BITS if min_correlation is None else min_correlation)
        if segment:
            self.set_segment(segment)

    def set_frame(self, frame, min_correlation=MIN_CORRELATION_BITS):
        """Symbols per frame (65 .. 2^20) and the acceptance; only before the first push."""
        _check(lib().xrit_framer_set_frame(self._h, int(frame), int(min_correlation)))
        self.frame = int(frame)

    def set_segment(self, chunks):
        """Chunks per walker segment (0: chosen per call).  The rows do not depend on it."""
        _check(lib().xrit_framer_set_segment(self._h, int(chunks)))

    def rows(self, n):
        """Rows the outputs of a push of n symbols must hold."""
        return int(lib().xrit_framer_rows(self._h, int(n)))

    def push(self, symbols, trim=True):
        """Host buffers: (frames (r, frame) int8, valid (r,) uint8, hits (r, 4) uint32 as the correlator found them,
        start (r,) uint64 absolute offsets) of the rows this call emits; trim = False: all rows(n) rows, those past the
        emitted ones all-zero, and the count as a fifth item."""
        d = np.ascontiguousarray(symbols, np.int8).reshape(-1)
        cap = self.rows(len(d))
        frames = np.zeros((cap, self.frame), np.int8)
        valid = np.zeros(cap, np.uint8)
        hits = np.zeros((cap, 4), np.uint32)
        start = np.zeros(cap, np.uint64)
        got = lib().xrit_framer_push(self._h, _p(d) if len(d) else None, len(d), _p(frames), _p(valid), _p(hits), _p(start))
        if got < 0:
            _check(got)
        if trim:
            return frames[:got], valid[:got], hits[:got], start[:got]
        return frames, valid, hits, start, got

    def push_device(self, d_symbols_ptr, n, d_frames_ptr, d_valid_ptr, d_hits_ptr, d_start_ptr, d_count_ptr, stream=None):
        """Device pointers (frames rows(n) * frame bytes, valid rows(n), hits rows(n) * 16, start rows(n) * 8, count 4
        bytes), asynchronous on stream; FrameDecoder.decode_device and ChannelDemux.process_device may be queued behind
        it with nf = rows(n)."""
        _check(lib().xrit_framer_push_device(self._h, C.c_void_p(d_symbols_ptr) if d_symbols_ptr else None, n,
                                             C.c_void_p(d_frames_ptr), C.c_void_p(d_valid_ptr), C.c_void_p(d_hits_ptr),
                                             C.c_void_p(d_start_ptr), C.c_void_p(d_count_ptr),
                                             C.c_void_p(stream) if stream else None))

    def stats(self):
        """The counters after the last call (a FRAMER_STATS_DTYPE scalar record); waits for that call."""
        out = np.zeros(1, FRAMER_STATS_DTYPE)
        _check(lib().xrit_framer_stats(self._h, _p(out)))
        return out[0]

    def reset(self):
        """Cursor 0, nothing carried, counters zero."""
        _check(lib().xrit_framer_reset(self._h))


# ---- decoder: Viterbi27 + NRZ-M + derandomiser + 4 x RS(255,223) (decoder/src/newdecoder.cpp:272-348) ------------
CADU_SIZE, BLOCK_SIZE, VCDU_SIZE = 1024, 1020, 892

# xrit_frame_info, one row per frame
FRAME_INFO_DTYPE = np.dtype([("valid", np.uint32), ("ok", np.uint32), ("viterbi_errors", np.uint32),
                             ("rs_errors", np.int32, (4,)), ("scid", np.uint32), ("vcid", np.uint32),
                             ("counter", np.uint32)])


class FrameDecoder(_Handle):
    """The decoder's per-frame FEC on aligned, phase-fixed frames (what sync_fix_frames returns): the Viterbi window
    (64 carried symbols + the frame), HRIT's NRZ-M, the derandomiser and four interleaved RS(255,223) codewords.  The
    carry runs across calls until reset().  mode: "lrit" or "hrit"."""
    _destroy = "xrit_decoder_destroy"

    def __init__(self, mode="lrit", device=0):
        super().__init__()
        if mode not in ("lrit", "hrit"):
            raise ValueError(f"mode {mode!r}: 'lrit' or 'hrit'")
        self.mode = mode
        _check(lib().xrit_decoder_create(C.byref(self._h), 1 if mode == "hrit" else 0, device))

    def decode(self, frames, valid):
        """frames (nf, 16384) int8, valid (nf,) -> (cadu (nf, 1024) uint8, block (nf, 1020) uint8, info (nf,)
        FRAME_INFO_DTYPE).  The VCDU of frame f is block[f, :892]; it counts when info["ok"][f]."""
        fr = np.ascontiguousarray(frames, np.int8).reshape(-1, CODED_FRAME_SIZE)
        v = np.ascontiguousarray(valid, np.uint8).reshape(-1)
        if len(v) != len(fr):
            raise ValueError(f"{len(fr)} frames but {len(v)} valid flags")
        nf = len(fr)
        cadu = np.zeros((nf, CADU_SIZE), np.uint8)
        block = np.zeros((nf, BLOCK_SIZE), np.uint8)
        info = np.zeros(nf, FRAME_INFO_DTYPE)
        _check(lib().xrit_decoder_decode(self._h, _p(fr), _p(v), nf, _p(cadu), _p(block), _p(info)))
        return cadu, block, info

    def decode_device(self, d_frames_ptr, d_valid_ptr, nf, d_cadu_ptr, d_block_ptr, d_info_ptr, stream=None):
        """Device pointers (cadu and block 16-byte aligned, info nf * FRAME_INFO_DTYPE.itemsize bytes), asynchronous on
        stream."""
        _check(lib().xrit_decoder_decode_device(self._h, C.c_void_p(d_frames_ptr), C.c_void_p(d_valid_ptr), nf,
                                                C.c_void_p(d_cadu_ptr), C.c_void_p(d_block_ptr), C.c_void_p(d_info_ptr),
                                                C.c_void_p(stream) if stream else None))

    def reset(self):
        """The carry back to erasures (the decoder's start state)."""
        _check(lib().xrit_decoder_reset(self._h))

    def set_windows(self, windows):
        """At most this many resident Viterbi windows per call from the next call on (0: the default, 8 per compute
        unit; clamped to 1 .. default).  The outputs do not depend on it."""
        _check(lib().xrit_decoder_set_windows(self._h, int(windows)))


# ---- frame lock: framer and decoder as the reference's one loop, with its flywheel (newdecoder.cpp:218-237, 321-338)
LOCK_FULL, LOCK_SHORT, LOCK_MISS, LOCK_RECHECK = 0, 1, 2, 4
FLYWHEEL_RECHECK = 4                 # decoder/src/parameters.h:41
# xrit_lock_counters: the framer's, then the loop's
LOCK_STATS_DTYPE = np.dtype(FRAMER_STATS_DTYPE.descr + [(f, np.uint64) for f in (
    "short_kept", "short_missed", "rechecks", "sensitive_chunks", "rounds", "frames_ok", "frames_bad")])
assert LOCK_STATS_DTYPE.itemsize == 136


class FrameLock(_Handle):
    """FrameSynchroniser and FrameDecoder as the one loop the reference runs: after a good frame (its Reed-Solomon
    outcome) only the first frame / 16 positions of the next chunk are correlated and position 0 is kept if it is the best
    of them; every `flywheel` chunks the whole chunk is correlated again.  flywheel = 1 is the framer followed by the
    decoder.  The rows do not depend on how the stream is cut into calls.  mode: "lrit" or "hrit"."""
    _destroy = "xrit_lock_destroy"

    def __init__(self, mode="lrit", device=0, flywheel=None, segment=0, windows=0):
        super().__init__()
        if mode not in ("lrit", "hrit"):
            raise ValueError(f"mode {mode!r}: 'lrit' or 'hrit'")
        self.mode = mode
        _check(lib().xrit_lock_create(C.byref(self._h), 1 if mode == "hrit" else 0, device))
        self.frame = CODED_FRAME_SIZE
        if flywheel is not None:
            self.set_flywheel(flywheel)
        if segment:
            self.set_segment(segment)
        if windows:
            self.set_windows(windows)

    def set_flywheel(self, recheck):
        """flywheelRecheck, 1 .. 255 (default 4); only before the first push."""
        if not 0 <= int(recheck) < 1 << 32:
            raise ValueError("flywheel recheck 1..255")
        _check(lib().xrit_lock_set_flywheel(self._h, int(recheck)))

    def set_segment(self, chunks):
        """Chunks per walker segment (0: chosen per call).  The outputs do not depend on it."""
        _check(lib().xrit_lock_set_segment(self._h, int(chunks)))

    def set_windows(self, windows):
        """Resident Viterbi windows a call uses at most (0: the default).  The outputs do not depend on it."""
        _check(lib().xrit_lock_set_windows(self._h, int(windows)))

    def rows(self, n):
        """Rows the outputs of a push of n symbols must hold."""
        return int(lib().xrit_lock_rows(self._h, int(n)))

    def push(self, symbols, trim=True):
        """Host buffers: (frames, valid, hits, start) as FrameSynchroniser.push gives them, mode (r,) uint8, and (cadu,
        block, info) as FrameDecoder.decode gives them, of the rows this call emits; trim = False: all rows(n) rows, those
        past the emitted ones absent, and the count as a ninth item."""
        d = np.ascontiguousarray(symbols, np.int8).reshape(-1)
        cap = self.rows(len(d))
        frames = np.zeros((cap, self.frame), np.int8)
        valid = np.zeros(cap, np.uint8)
        hits = np.zeros((cap, 4), np.uint32)
        start = np.zeros(cap, np.uint64)
        mode = np.zeros(cap, np.uint8)
        cadu = np.zeros((cap, CADU_SIZE), np.uint8)
        block = np.zeros((cap, BLOCK_SIZE), np.uint8)
        info = np.zeros(cap, FRAME_INFO_DTYPE)
        got = lib().xrit_lock_push(self._h, _p(d) if len(d) else None, len(d), _p(frames), _p(valid), _p(hits), _p(start),
                                   _p(mode), _p(cadu), _p(block), _p(info))
        if got < 0:
            _check(got)
        out = (frames, valid, hits, start, mode, cadu, block, info)
        if trim:
            return tuple(a[:got] for a in out)
        return out + (got,)

    def push_device(self, d_symbols_ptr, n, d_frames_ptr, d_valid_ptr, d_hits_ptr, d_start_ptr, d_mode_ptr, d_cadu_ptr,
                    d_block_ptr, d_info_ptr, d_count_ptr, stream=None):
        """Device pointers, rows(n) rows each (cadu 16-byte aligned).  Queued on stream, which the call synchronises once
        per round; ChannelDemux.process_device takes hits, cadu, block and info as they are with nf = rows(n)."""
        ptrs = (d_frames_ptr, d_valid_ptr, d_hits_ptr, d_start_ptr, d_mode_ptr, d_cadu_ptr, d_block_ptr, d_info_ptr, d_count_ptr)
        _check(lib().xrit_lock_push_device(self._h, C.c_void_p(d_symbols_ptr) if d_symbols_ptr else None, n,
                                           *(C.c_void_p(q) if q else None for q in ptrs),
                                           C.c_void_p(stream) if stream else None))

    def stats(self):
        """The counters after the last call (a LOCK_STATS_DTYPE scalar record); waits for that call."""
        out = np.zeros(1, LOCK_STATS_DTYPE)
        _check(lib().xrit_lock_stats(self._h, _p(out)))
        return out[0]

    def reset(self):
        """Cursor 0, nothing carried, ok and fc cleared, the decoder's carry back to erasures, counters zero."""
        _check(lib().xrit_lock_reset(self._h))


# ---- channel demultiplexer and packet accounting (decoder/src/newdecoder.cpp:309-395) -------------------------------
N_VCID = 64
STATISTICS_WIRE_BYTES = 4167         # sizeof(Statistics_st), packed (decoder/src/Statistics.h:14-36)

# xrit_frame_stats: Statistics_st after one frame, without the arrays (one row per frame)
FRAME_STATS_DTYPE = np.dtype([
    ("packet_number", np.uint64), ("lost_packets", np.uint64), ("dropped_packets", np.uint64),
    ("total_packets", np.uint64), ("received_vc", np.int64), ("lost_vc", np.int64),
    ("rs_errors", np.int32, (4,)),
    ("vit_errors", np.uint16), ("frame_bits", np.uint16), ("average_vit_corrections", np.uint16),
    ("scid", np.uint8), ("vcid", np.uint8), ("signal_quality", np.uint8), ("sync_correlation", np.uint8),
    ("phase_correction", np.uint8), ("average_rs_corrections", np.uint8), ("sync_word", np.uint8, (4,)),
    ("frame_lock", np.uint8), ("valid", np.uint8), ("reserved", np.uint8, (6,))])
assert FRAME_STATS_DTYPE.itemsize == 88

# xrit_decoder_stats: the counters of newdecoder.cpp:44-53 after a call
DECODER_STATS_DTYPE = np.dtype([
    ("total_packets", np.uint64), ("dropped_packets", np.uint64), ("lost_packets", np.uint64),
    ("sum_viterbi_errors", np.uint64), ("sum_rs_corrections", np.uint64),
    ("received", np.int64, (256,)), ("lost", np.int64, (256,)), ("last_counter", np.int64, (256,)),
    ("start_time", np.uint32), ("reserved", np.uint32)])
assert DECODER_STATS_DTYPE.itemsize == 6192


def _hits16(hits, nf):
    h = np.zeros((nf, 4), np.uint32)
    if nf:
        a = np.asarray(hits, np.uint32).reshape(nf, -1)
        h[:, :min(4, a.shape[1])] = a[:, :4]
    return h


class ChannelDemux(_Handle):
    """The reference decoder's last stage on the frame decoder's outputs: the good frames' VCDUs split by virtual
    channel (ChannelWriter::writeChannel) and the Statistics_st record of every valid frame (newdecoder.cpp:309-395).
    The counters run across calls until reset()."""
    _destroy = "xrit_demux_destroy"

    def __init__(self, device=0):
        super().__init__()
        _check(lib().xrit_demux_create(C.byref(self._h), device))

    def process(self, hits, cadu, block, info):
        """hits: rows (word, position, correlation[, reserved]) as the correlator returned them; cadu (nf, 1024),
        block (nf, 1020), info (nf,) FRAME_INFO_DTYPE as FrameDecoder.decode returns them.  -> (vcdu (n_good, 892)
        uint8 grouped by VCID in ascending order, frame order within a VCID; offsets (65,) uint32, channel v's rows
        are offsets[v]:offsets[v + 1]; records (nf,) FRAME_STATS_DTYPE)."""
        info = np.ascontiguousarray(info, FRAME_INFO_DTYPE).reshape(-1)
        nf = len(info)
        cadu = np.ascontiguousarray(cadu, np.uint8).reshape(nf, CADU_SIZE)
        block = np.ascontiguousarray(block, np.uint8).reshape(nf, BLOCK_SIZE)
        h = _hits16(hits, nf)
        good = int(((info["valid"] != 0) & (info["ok"] != 0)).sum())
        vcdu = np.zeros((good, VCDU_SIZE), np.uint8)
        offsets = np.zeros(N_VCID + 1, np.uint32)
        records = np.zeros(nf, FRAME_STATS_DTYPE)
        _check(lib().xrit_demux_process(self._h, _p(h), _p(cadu), _p(block), _p(info), nf, _p(vcdu), _p(offsets),
                                        _p(records)))
        return vcdu, offsets, records

    def channels(self, hits, cadu, block, info):
        """process(), split: {vcid: (n, 892) uint8} for every VCID with good frames in this call."""
        vcdu, off, _ = self.process(hits, cadu, block, info)
        return {v: vcdu[off[v]:off[v + 1]] for v in range(N_VCID) if off[v + 1] > off[v]}

    def process_device(self, d_hits_ptr, d_cadu_ptr, d_block_ptr, d_info_ptr, nf, d_vcdu_ptr, d_offsets_ptr,
                       d_records_ptr, stream=None):
        """Device pointers (hits nf x 16 bytes, cadu nf x 1024, block nf x 1020, info nf x 40, vcdu room for nf x 892,
        offsets 65 x 4, records nf x 88), asynchronous on stream; may be queued behind FrameDecoder.decode_device."""
        _check(lib().xrit_demux_process_device(self._h, C.c_void_p(d_hits_ptr), C.c_void_p(d_cadu_ptr),
                                               C.c_void_p(d_block_ptr), C.c_void_p(d_info_ptr), nf,
                                               C.c_void_p(d_vcdu_ptr), C.c_void_p(d_offsets_ptr),
                                               C.c_void_p(d_records_ptr), C.c_void_p(stream) if stream else None))

    def stats(self):
        """The counters after the last call (a DECODER_STATS_DTYPE scalar record); waits for that call."""
        out = np.zeros(1, DECODER_STATS_DTYPE)
        _check(lib().xrit_demux_stats(self._h, _p(out)))
        return out[0]

    @staticmethod
    def wire_records(start, records):
        """The Statistics_st stream StatisticsDispatcher would send for one call: `start` is stats() taken before the
        call, `records` the call's records; one 4167-byte record per valid frame, as bytes."""
        st = np.zeros(1, DECODER_STATS_DTYPE)
        st[0] = start
        rec = np.ascontiguousarray(records, FRAME_STATS_DTYPE).reshape(-1)
        n = int((rec["valid"] != 0).sum())
        out = np.zeros(max(n, 1) * STATISTICS_WIRE_BYTES, np.uint8)
        got = lib().xrit_demux_expand(_p(st), _p(rec), len(rec), _p(out))
        if got < 0:
            _check(got)
        assert got == n
        return out[:n * STATISTICS_WIRE_BYTES].tobytes()

    def reset(self):
        """The start state of newdecoder.cpp:133-137 (startTime is kept)."""
        _check(lib().xrit_demux_reset(self._h))


# ---- packet assembler: CCSDS space packets out of the demultiplexed VCDUs, with CRC -----------
# xrit_packet: one descriptor per emitted packet
PACKET_DTYPE = np.dtype([
    ("offset", np.uint64), ("length", np.uint32), ("first_counter", np.uint32),
    ("apid", np.uint16), ("seq_count", np.uint16), ("crc_computed", np.uint16), ("crc_carried", np.uint16),
    ("vcid", np.uint8), ("seq_flags", np.uint8), ("crc_ok", np.uint8), ("header_bits", np.uint8),
    ("reserved", np.uint8, (4,))])
assert PACKET_DTYPE.itemsize == 32

# xrit_packets_summary: a call's true counts and the handle's counters after it
PACKETS_SUMMARY_DTYPE = np.dtype([
    ("packets", np.uint64), ("bytes", np.uint64),
    ("total_packets", np.uint64), ("crc_failures", np.uint64), ("fill_packets", np.uint64), ("discarded", np.uint64),
    ("bad_fhp", np.uint64), ("rows", np.uint64), ("overflow", np.uint32), ("reserved", np.uint32)])
assert PACKETS_SUMMARY_DTYPE.itemsize == 72

# xrit_packets_counters: the full counters, per channel included
PACKETS_STATS_DTYPE = np.dtype([
    ("packets", np.uint64), ("crc_failures", np.uint64), ("fill_packets", np.uint64), ("discarded", np.uint64),
    ("bad_fhp", np.uint64), ("rows", np.uint64),
    ("vc_packets", np.uint64, (64,)), ("vc_crc_failures", np.uint64, (64,)), ("vc_fill_packets", np.uint64, (64,)),
    ("vc_discarded", np.uint64, (64,)), ("vc_bad_fhp", np.uint64, (64,)), ("vc_rows", np.uint64, (64,)),
    ("last_counter", np.int64, (64,)), ("pending_bytes", np.uint32, (64,)), ("pending_first_counter", np.uint32, (64,))])
assert PACKETS_STATS_DTYPE.itemsize == 4144

PACKET_ZONE = 884                    # bytes of M_PDU packet zone in a VCDU
PACKET_MAX = 65542                   # the longest space packet, primary header included


def packets_max_bytes(rows):
    """No call on `rows` rows emits more bytes than this (XRIT_PACKETS_MAX_BYTES)."""
    return PACKET_ZONE * rows + (PACKET_MAX - 1) * N_VCID


class PacketAssembler(_Handle):
    """CCSDS space packets (the LRIT/HRIT CP_PDUs) out of ChannelDemux's rows: per channel the M_PDU first header
    pointer is followed, a packet under which a VCDU was lost is dropped, every other one is emitted whole with its
    CRC-16 checked.  What has begun and not ended is carried across calls until reset()."""
    _destroy = "xrit_packets_destroy"

    def __init__(self, device=0):
        super().__init__()
        _check(lib().xrit_packets_create(C.byref(self._h), device))

    def process(self, vcdu, offsets, max_packets=None, max_bytes=None):
        """vcdu (n, 892) uint8 and offsets (65,) uint32 as ChannelDemux.process returns them.  -> (bytes uint8: the
        emitted packets back to back, VCID ascending, stream order within a VCID; packets (n_packets,) PACKET_DTYPE;
        pkt_offsets (65,) uint32: channel v's packets are pkt_offsets[v]:pkt_offsets[v + 1]; summary, a
        PACKETS_SUMMARY_DTYPE record).  With capacities that turn out too small XritError -5 is raised; its `partial`
        holds the same four with the prefix that fitted (the handle's state has advanced all the same)."""
        offsets = np.ascontiguousarray(offsets, np.uint32).reshape(N_VCID + 1)
        rows = int(offsets[N_VCID])
        vcdu = np.ascontiguousarray(vcdu, np.uint8).reshape(-1, VCDU_SIZE)
        if len(vcdu) < rows:
            raise ValueError("offsets[64] counts more rows than vcdu holds")
        cap_b = packets_max_bytes(rows) if max_bytes is None else int(max_bytes)
        cap_p = 127 * rows + N_VCID if max_packets is None else int(max_packets)
        buf = np.empty(max(cap_b, 1), np.uint8)              # (untouched pages cost nothing)
        desc = np.empty(max(cap_p, 1), PACKET_DTYPE)
        pkt_offsets = np.zeros(N_VCID + 1, np.uint32)
        summary = np.zeros(1, PACKETS_SUMMARY_DTYPE)
        rc = lib().xrit_packets_process(self._h, _p(vcdu), _p(offsets), _p(buf), cap_b, _p(desc), cap_p, _p(pkt_offsets),
                                        _p(summary))
        if rc not in (0, -5):
            _check(rc)
        n = min(int(summary[0]["packets"]), cap_p)
        desc = desc[:n].copy()
        if int(summary[0]["bytes"]) <= cap_b:
            nb = int(summary[0]["bytes"])
        else:                                                # whole packets only: up to the end of the last one that fits
            ends = desc["offset"] + desc["length"]
            ends = ends[ends <= cap_b]
            nb = int(ends[-1]) if len(ends) else 0
        out = (buf[:nb].copy(), desc, pkt_offsets, summary[0])
        if rc != 0:
            err = XritError(rc, lib().xrit_last_error().decode("utf-8", "replace"))
            err.partial = out
            raise err
        return out

    def process_device(self, d_vcdu_ptr, d_offsets_ptr, max_rows, d_bytes_ptr, max_bytes, d_packets_ptr, max_packets,
                       d_pkt_offsets_ptr, d_summary_ptr, stream=None):
        """Device pointers (vcdu rows of 892 bytes and offsets 65 x 4 as ChannelDemux.process_device wrote them, bytes
        max_bytes, packets max_packets x 32, pkt_offsets 65 x 4, summary 72 bytes), asynchronous on stream; may be
        queued behind ChannelDemux.process_device: the row count is read from offsets[64] on the device, max_rows is
        the host's bound on it (that call's nf)."""
        _check(lib().xrit_packets_process_device(self._h, C.c_void_p(d_vcdu_ptr), C.c_void_p(d_offsets_ptr), max_rows,
                                                 C.c_void_p(d_bytes_ptr), max_bytes, C.c_void_p(d_packets_ptr),
                                                 max_packets, C.c_void_p(d_pkt_offsets_ptr), C.c_void_p(d_summary_ptr),
                                                 C.c_void_p(stream) if stream else None))

    @staticmethod
    def split(data, packets):
        """The packets of one call as a list of bytes objects, in order."""
        raw = np.asarray(data, np.uint8).tobytes()
        return [raw[int(o):int(o) + int(n)] for o, n in zip(packets["offset"], packets["length"])]

    def stats(self):
        """The counters after the last call (a PACKETS_STATS_DTYPE scalar record); waits for that call."""
        out = np.zeros(1, PACKETS_STATS_DTYPE)
        _check(lib().xrit_packets_stats(self._h, _p(out)))
        return out[0]

    def reset(self):
        """Every channel back to its start: no last counter, nothing pending, counters zero."""
        _check(lib().xrit_packets_reset(self._h))


# ---- file assembler and Rice decoder (DESIGN.md sections 15 and 16) ---------------------------------------------------
# xrit_file_piece: one descriptor per emitted piece (offset and length lie as in xrit_packet)
FILE_PIECE_DTYPE = np.dtype([
    ("offset", np.uint64), ("length", np.uint32), ("index_in_file", np.uint32), ("file", np.uint32),
    ("seq_count", np.uint16), ("apid", np.uint16), ("vcid", np.uint8), ("seq_flags", np.uint8), ("reserved", np.uint8, (6,))])
assert FILE_PIECE_DTYPE.itemsize == 32

# xrit_file_record: one per file touched in a call
FILE_RECORD_DTYPE = np.dtype([
    ("offset", np.uint64), ("length", np.uint64), ("file_offset", np.uint64), ("declared_bits", np.uint64),
    ("data_bits", np.uint64),
    ("header_length", np.uint32), ("first_piece", np.uint32), ("n_pieces", np.uint32), ("key_serial", np.uint32),
    ("file_counter", np.uint16), ("apid", np.uint16), ("columns", np.uint16), ("lines", np.uint16), ("rice_flags", np.uint16),
    ("vcid", np.uint8), ("flags", np.uint8), ("file_type", np.uint8), ("header_state", np.uint8),
    ("bits_per_pixel", np.uint8), ("compression", np.uint8), ("pixels_per_block", np.uint8), ("lines_per_packet", np.uint8),
    ("reserved", np.uint8, (6,))])
assert FILE_RECORD_DTYPE.itemsize == 80
FILE_BEGINS, FILE_ENDS, FILE_ABORTED, FILE_LENGTH_MATCH = 1, 2, 4, 8

_FILES_COUNTERS = [(k, np.uint64) for k in ("files_begun", "files_completed", "files_aborted", "bad_packets", "seq_gaps",
                                            "short_first", "orphans", "total_pieces", "total_bytes")]
# xrit_files_summary: a call's true counts and the handle's counters after it
FILES_SUMMARY_DTYPE = np.dtype([("pieces", np.uint64), ("bytes", np.uint64), ("files", np.uint64)] + _FILES_COUNTERS +
                               [("overflow", np.uint32), ("reserved", np.uint32)])
assert FILES_SUMMARY_DTYPE.itemsize == 104
# xrit_files_counters
FILES_STATS_DTYPE = np.dtype(_FILES_COUNTERS + [("open_files", np.uint64)])
assert FILES_STATS_DTYPE.itemsize == 80
# xrit_file_key: what one (vcid, apid) carries
FILE_KEY_DTYPE = np.dtype([
    ("file_bytes", np.uint64), ("declared_bits", np.uint64), ("data_bits", np.uint64),
    ("header_length", np.uint32), ("n_pieces", np.uint32), ("key_serial", np.uint32),
    ("next_seq", np.uint16), ("file_counter", np.uint16), ("columns", np.uint16), ("lines", np.uint16), ("rice_flags", np.uint16),
    ("open", np.uint8), ("file_type", np.uint8), ("header_state", np.uint8), ("bits_per_pixel", np.uint8),
    ("compression", np.uint8), ("pixels_per_block", np.uint8), ("lines_per_packet", np.uint8), ("reserved", np.uint8, (3,))])
assert FILE_KEY_DTYPE.itemsize == 56


class FileAssembler(_Handle):
    """LRIT/HRIT files out of PacketAssembler's packets: per (vcid, apid) the sequence flags and counts are followed and
    the transport header and the header records of a file's first packet parsed; a call emits the pieces it saw and one
    record per file touched, and the host appends.  What is open is carried across calls until reset()."""
    _destroy = "xrit_files_destroy"

    def __init__(self, device=0):
        super().__init__()
        _check(lib().xrit_files_create(C.byref(self._h), device))

    def process(self, data, packets, pkt_offsets, max_bytes=None, max_pieces=None, max_files=None):
        """data uint8, packets PACKET_DTYPE and pkt_offsets (65,) uint32 as PacketAssembler.process returns them.  ->
        (bytes uint8: the emitted payloads back to back; pieces FILE_PIECE_DTYPE; files FILE_RECORD_DTYPE; summary, a
        FILES_SUMMARY_DTYPE record), all ordered by (vcid, apid, stream order).  With capacities that turn out too small
        XritError -5 is raised; its `partial` holds the same four with the prefix that fitted (the handle's state has
        advanced all the same)."""
        pkt_offsets = np.ascontiguousarray(pkt_offsets, np.uint32).reshape(N_VCID + 1)
        n = int(pkt_offsets[N_VCID])
        data = np.ascontiguousarray(data, np.uint8).reshape(-1)
        packets = np.ascontiguousarray(packets, PACKET_DTYPE).reshape(-1)
        if len(packets) < n:
            raise ValueError("pkt_offsets[64] counts more packets than there are descriptors")
        cap_b = len(data) if max_bytes is None else int(max_bytes)
        cap_p = n if max_pieces is None else int(max_pieces)
        cap_f = 2 * n if max_files is None else int(max_files)
        buf = np.empty(max(cap_b, 1), np.uint8)
        pieces = np.empty(max(cap_p, 1), FILE_PIECE_DTYPE)
        files = np.empty(max(cap_f, 1), FILE_RECORD_DTYPE)
        summary = np.zeros(1, FILES_SUMMARY_DTYPE)
        rc = lib().xrit_files_process(self._h, _p(data), len(data), _p(packets), _p(pkt_offsets), _p(buf), cap_b, _p(pieces),
                                      cap_p, _p(files), cap_f, _p(summary))
        if rc not in (0, -5):
            _check(rc)
        pieces = pieces[:min(int(summary[0]["pieces"]), cap_p)].copy()
        files = files[:min(int(summary[0]["files"]), cap_f)].copy()
        if int(summary[0]["bytes"]) <= cap_b:
            nb = int(summary[0]["bytes"])
        else:                                                # whole pieces only: up to the end of the last one that fits
            ends = pieces["offset"] + pieces["length"]
            ends = ends[ends <= cap_b]
            nb = int(ends[-1]) if len(ends) else 0
        out = (buf[:nb].copy(), pieces, files, summary[0])
        if rc != 0:
            err = XritError(rc, lib().xrit_last_error().decode("utf-8", "replace"))
            err.partial = out
            raise err
        return out

    def process_device(self, d_in_bytes_ptr, in_bytes, d_packets_ptr, d_pkt_offsets_ptr, max_packets_in, d_bytes_ptr, max_bytes,
                       d_pieces_ptr, max_pieces, d_files_ptr, max_files, d_summary_ptr, stream=None):
        """Device pointers (bytes of in_bytes, packets max_packets_in x 32 and pkt_offsets 65 x 4 as
        PacketAssembler.process_device wrote them; bytes max_bytes, pieces max_pieces x 32, files max_files x 80,
        summary 104 bytes), asynchronous on stream; may be queued behind PacketAssembler.process_device: the packet
        count is read from pkt_offsets[64] on the device, max_packets_in is the host's bound on it."""
        _check(lib().xrit_files_process_device(self._h, C.c_void_p(d_in_bytes_ptr), in_bytes, C.c_void_p(d_packets_ptr),
                                               C.c_void_p(d_pkt_offsets_ptr), max_packets_in, C.c_void_p(d_bytes_ptr), max_bytes,
                                               C.c_void_p(d_pieces_ptr), max_pieces, C.c_void_p(d_files_ptr), max_files,
                                               C.c_void_p(d_summary_ptr), C.c_void_p(stream) if stream else None))

    def stats(self):
        """The counters after the last call (a FILES_STATS_DTYPE scalar record); waits for that call."""
        out = np.zeros(1, FILES_STATS_DTYPE)
        _check(lib().xrit_files_stats(self._h, _p(out)))
        return out[0]

    def key(self, vcid, apid):
        """What (vcid, apid) carries after the last call (a FILE_KEY_DTYPE scalar record); waits for that call."""
        out = np.zeros(1, FILE_KEY_DTYPE)
        _check(lib().xrit_files_key(self._h, vcid, apid, _p(out)))
        return out[0]

    def reset(self):
        """Every key back to its start: nothing open, serials and counters zero."""
        _check(lib().xrit_files_reset(self._h))


RICE_FORMS = {"default": 0, "lane": 1, "wave": 2}


def rice_form(form="default"):
    """Which kernel RiceDecoder launches from now on, process wide: "default" (the wave form), "lane" (one lane per
    line) or "wave" (one wave per line).  Both are held to the same specification."""
    _check(lib().xrit_rice_form(RICE_FORMS[form]))


class RiceDecoder:
    """The Rice decoder (CCSDS 121.0-B) on batches of coded lines: bits per sample 1 .. 16, block 8 / 16 / 32 / 64,
    samples per line 1 .. 65535.  Stateless."""

    def __init__(self, bits_per_sample, block, samples, device=0):
        self.n, self.J, self.S, self.device = int(bits_per_sample), int(block), int(samples), device
        # an empty batch: the parameters and the device are checked here, not at the first line
        _check(lib().xrit_rice_decode(None, 0, None, 16, 0, self.n, self.J, self.S, None, None, device))

    def decode(self, data, desc):
        """data uint8; desc a structured array whose records begin {offset u64, length u32} (PACKET_DTYPE,
        FILE_PIECE_DTYPE or tests' 16-byte form), one line each.  -> (samples (n_lines, S) uint8 or uint16,
        status (n_lines,) uint8: 0, 1 a fault -- whole blocks kept, the rest 0 --, 2 descriptor outside data)."""
        data = np.ascontiguousarray(data, np.uint8).reshape(-1)
        desc = np.ascontiguousarray(desc).reshape(-1)
        out = np.zeros((len(desc), self.S), np.uint8 if self.n <= 8 else np.uint16)
        status = np.zeros(len(desc), np.uint8)
        _check(lib().xrit_rice_decode(_p(data), len(data), _p(desc), desc.dtype.itemsize, len(desc), self.n, self.J, self.S,
                                      _p(out), _p(status), self.device))
        return out, status

    def decode_device(self, d_bytes_ptr, n_bytes, d_desc_ptr, stride, n_lines, d_out_ptr, d_status_ptr, stream=None):
        """Device pointers, asynchronous on stream."""
        _check(lib().xrit_rice_decode_device(C.c_void_p(d_bytes_ptr), n_bytes, C.c_void_p(d_desc_ptr), stride, n_lines, self.n,
                                             self.J, self.S, C.c_void_p(d_out_ptr), C.c_void_p(d_status_ptr), self.device,
                                             C.c_void_p(stream) if stream else None))


def is_rice_coded(record, first_piece_length):
    """The link between the two stages (this project's convention): the record's file is an image
    whose first piece carries the headers alone and whose pieces 1, 2, ... are one Rice-coded line each."""
    return (int(record["header_state"]) == 2 and int(record["file_type"]) == 0 and int(record["compression"]) == 1 and
            1 <= int(record["bits_per_pixel"]) <= 16 and int(record["columns"]) >= 1 and
            int(record["pixels_per_block"]) in (8, 16, 32, 64) and int(record["header_length"]) == int(first_piece_length))


def decode_file_lines(record, pieces, data, device=0):
    """The scan lines of a rice-coded file whose pieces all lie in one call: record, a FILE_RECORD_DTYPE with BEGINS;
    pieces and data, that call's.  -> (samples (n_pieces - 1, columns), status) or None when the link rule says the file
    is not rice-coded."""
    mine = pieces[int(record["first_piece"]):int(record["first_piece"]) + int(record["n_pieces"])]
    if not (int(record["flags"]) & FILE_BEGINS) or len(mine) < 1 or not is_rice_coded(record, mine[0]["length"]):
        return None
    dec = RiceDecoder(int(record["bits_per_pixel"]), int(record["pixels_per_block"]), int(record["columns"]), device)
    return dec.decode(data, mine[1:])


# ---- image lines ---------------------------------------------------------------------------------
# xrit_image_line: one per decoded line (offset and length lie as in xrit_packet)
IMAGE_LINE_DTYPE = np.dtype([
    ("offset", np.uint64), ("length", np.uint32), ("row", np.uint32), ("file", np.uint32), ("piece", np.uint32),
    ("samples", np.uint16), ("bits", np.uint8), ("status", np.uint8), ("reserved", np.uint8, (4,))])
assert IMAGE_LINE_DTYPE.itemsize == 32
# xrit_image_file: one per files record, all zero where the record is not a rice-coded image's
IMAGE_FILE_DTYPE = np.dtype([
    ("offset", np.uint64), ("length", np.uint64), ("first_line", np.uint32), ("n_lines", np.uint32), ("first_row", np.uint32),
    ("faults", np.uint32), ("lines_total", np.uint32), ("faults_total", np.uint32), ("columns", np.uint16), ("bits", np.uint8),
    ("rice", np.uint8), ("reserved", np.uint8, (4,))])
assert IMAGE_FILE_DTYPE.itemsize == 48
_IMAGES_COUNTERS = [(k, np.uint64) for k in ("images_begun", "images_completed", "images_aborted", "total_lines", "total_faults",
                                             "total_bytes")]
# xrit_images_summary: a call's true counts and the handle's counters after it
IMAGES_SUMMARY_DTYPE = np.dtype([("lines", np.uint64), ("bytes", np.uint64), ("images", np.uint64)] + _IMAGES_COUNTERS +
                                [("overflow", np.uint32), ("reserved", np.uint32)])
assert IMAGES_SUMMARY_DTYPE.itemsize == 80
# xrit_images_counters
IMAGES_STATS_DTYPE = np.dtype(_IMAGES_COUNTERS)
assert IMAGES_STATS_DTYPE.itemsize == 48
# xrit_image_key: what one (vcid, apid) carries
IMAGE_KEY_DTYPE = np.dtype([("key_serial", np.uint32), ("lines", np.uint32), ("faults", np.uint32), ("open", np.uint8),
                            ("reserved", np.uint8, (3,))])
assert IMAGE_KEY_DTYPE.itemsize == 16


def images_max_bytes(files):
    """A bound on the image bytes of a call from its records (FILE_RECORD_DTYPE, on the host): every piece of a record a
    line of the record's width, padded to a multiple of 4."""
    files = np.asarray(files)
    width = np.where(files["bits_per_pixel"] <= 8, 1, 2).astype(np.int64)
    line = (files["columns"].astype(np.int64) * width + 3) & ~3
    return int((files["n_pieces"].astype(np.int64) * line).sum())


class ImageDecoder(_Handle):
    """Every Rice-coded line of every image file of one FileAssembler call, decoded in one pass: the images may differ
    in bits per pixel, block size and width.  Which images are open, with their lines and faults so far, is carried per
    (vcid, apid) across calls until reset(), so an image whose packets arrive over many calls needs nothing from the
    host but appending rows."""
    _destroy = "xrit_images_destroy"

    def __init__(self, device=0):
        super().__init__()
        _check(lib().xrit_images_create(C.byref(self._h), device))

    def process(self, data, pieces, files, summary, max_lines=None, max_bytes=None):
        """data, pieces, files and summary as FileAssembler.process returned them.  -> (bytes uint8: the lines' samples
        back to back, uint8 or little-endian uint16, every line padded to a multiple of 4 bytes; lines IMAGE_LINE_DTYPE;
        image_files IMAGE_FILE_DTYPE, one per record of `files`; summary, an IMAGES_SUMMARY_DTYPE record).  With
        capacities that turn out too small XritError -5 is raised; its `partial` holds the same four with the prefix
        that fitted (the handle's state has advanced all the same).  A files summary with overflow != 0, or with counts
        beyond len(pieces) / len(files), is refused: XritError -1, `partial` with the summary (overflow 2) alone, the
        state unchanged."""
        data = np.ascontiguousarray(data, np.uint8).reshape(-1)
        pieces = np.ascontiguousarray(pieces, FILE_PIECE_DTYPE).reshape(-1)
        files = np.ascontiguousarray(files, FILE_RECORD_DTYPE).reshape(-1)
        fsum = np.ascontiguousarray(np.asarray(summary, FILES_SUMMARY_DTYPE).reshape(1))
        cap_l = len(pieces) if max_lines is None else int(max_lines)
        cap_b = images_max_bytes(files) if max_bytes is None else int(max_bytes)
        buf = np.empty(max(cap_b, 1), np.uint8)
        lines = np.empty(max(cap_l, 1), IMAGE_LINE_DTYPE)
        ifiles = np.empty(max(len(files), 1), IMAGE_FILE_DTYPE)
        out_sum = np.zeros(1, IMAGES_SUMMARY_DTYPE)
        rc = lib().xrit_images_process(self._h, _p(data), len(data), _p(pieces), len(pieces), _p(files), len(files), _p(fsum),
                                       _p(buf), cap_b, _p(lines), cap_l, _p(ifiles), _p(out_sum))
        if rc != 0 and int(out_sum[0]["overflow"]) == 2:
            err = XritError(rc, lib().xrit_last_error().decode("utf-8", "replace"))
            err.partial = (buf[:0].copy(), lines[:0].copy(), ifiles[:0].copy(), out_sum[0])
            raise err
        if rc not in (0, -5):
            _check(rc)
        lines = lines[:min(int(out_sum[0]["lines"]), cap_l)].copy()
        ifiles = ifiles[:len(files)].copy()
        if int(out_sum[0]["bytes"]) <= cap_b:
            nb = int(out_sum[0]["bytes"])
        else:                                                # whole lines only: up to the end of the last one that fits
            ends = lines["offset"] + ((lines["length"].astype(np.uint64) + 3) & ~np.uint64(3))
            ends = ends[ends <= cap_b]
            nb = int(ends.max()) if len(ends) else 0
        out = (buf[:nb].copy(), lines, ifiles, out_sum[0])
        if rc != 0:
            err = XritError(rc, lib().xrit_last_error().decode("utf-8", "replace"))
            err.partial = out
            raise err
        return out

    def process_device(self, d_bytes_ptr, n_bytes, d_pieces_ptr, max_pieces_in, d_files_ptr, max_files_in, d_files_summary_ptr,
                       d_out_ptr, max_bytes, d_lines_ptr, max_lines, d_image_files_ptr, d_summary_ptr, stream=None):
        """Device pointers (bytes of n_bytes, pieces max_pieces_in x 32, files max_files_in x 80 and the 104-byte summary
        as FileAssembler.process_device wrote them; out max_bytes, lines max_lines x 32, image files max_files_in x 48,
        summary 80 bytes), asynchronous on stream; may be queued behind FileAssembler.process_device: the counts are
        read from its summary on the device."""
        _check(lib().xrit_images_process_device(self._h, C.c_void_p(d_bytes_ptr), n_bytes, C.c_void_p(d_pieces_ptr), max_pieces_in,
                                                C.c_void_p(d_files_ptr), max_files_in, C.c_void_p(d_files_summary_ptr),
                                                C.c_void_p(d_out_ptr), max_bytes, C.c_void_p(d_lines_ptr), max_lines,
                                                C.c_void_p(d_image_files_ptr), C.c_void_p(d_summary_ptr),
                                                C.c_void_p(stream) if stream else None))

    @staticmethod
    def rows(data, lines):
        """The lines' samples: a list of (uint8 or uint16 array of `samples` entries) per IMAGE_LINE_DTYPE record."""
        raw = np.asarray(data, np.uint8)
        out = []
        for ln in lines:
            a = raw[int(ln["offset"]):int(ln["offset"]) + int(ln["length"])]
            out.append(a.copy() if ln["bits"] <= 8 else a.view("<u2").copy())
        return out

    def stats(self):
        """The counters after the last call (an IMAGES_STATS_DTYPE scalar record); waits for that call."""
        out = np.zeros(1, IMAGES_STATS_DTYPE)
        _check(lib().xrit_images_stats(self._h, _p(out)))
        return out[0]

    def key(self, vcid, apid):
        """What (vcid, apid) carries after the last call (an IMAGE_KEY_DTYPE scalar record); waits for that call."""
        out = np.zeros(1, IMAGE_KEY_DTYPE)
        _check(lib().xrit_images_key(self._h, vcid, apid, _p(out)))
        return out[0]

    def reset(self):
        """Every key closed, counters zero."""
        _check(lib().xrit_images_reset(self._h))


# ---- image canvases ------------------------------------------------------------------------------
CANVAS_REASONS = ("NOT_RICE", "PLACED", "BAD_SEGMENT", "TOO_LARGE", "DUPLICATE", "OVERLAP", "NO_SLOT", "NO_PLACEMENT")
# xrit_canvas_file: one per files record, all zero where the record is not a rice-coded image's
CANVAS_FILE_DTYPE = np.dtype([
    ("slot", np.int32), ("reason", np.uint32), ("segment", np.uint32), ("start_line", np.uint32), ("start_column", np.uint32),
    ("lines_placed", np.uint32), ("lines_clipped", np.uint32), ("faults", np.uint32)])
assert CANVAS_FILE_DTYPE.itemsize == 32
# xrit_canvas_slot: one per canvas of the pool
CANVAS_SLOT_DTYPE = np.dtype([
    ("begun_mask", np.uint64), ("done_mask", np.uint64), ("aborted_mask", np.uint64),
    ("image_id", np.uint32), ("max_column", np.uint32), ("max_row", np.uint32), ("max_segment", np.uint32), ("pitch", np.uint32),
    ("lines_placed", np.uint32), ("faults", np.uint32), ("generation", np.uint32), ("born_call", np.uint32),
    ("touched_call", np.uint32),
    ("in_use", np.uint8), ("complete", np.uint8), ("vcid", np.uint8), ("bits", np.uint8), ("reserved", np.uint8, (4,)),
    ("name", np.uint8, (64,))])
assert CANVAS_SLOT_DTYPE.itemsize == 136
# xrit_canvas_segment: 64 per slot, entry segment - 1
CANVAS_SEGMENT_DTYPE = np.dtype([
    ("start_line", np.uint32), ("start_column", np.uint32), ("lines", np.uint32), ("columns", np.uint32), ("placed", np.uint32),
    ("faults", np.uint32), ("key_serial", np.uint32), ("apid", np.uint16), ("begun", np.uint8), ("reserved", np.uint8)])
assert CANVAS_SEGMENT_DTYPE.itemsize == 32
# xrit_canvas_key_state: what one (vcid, apid) carries
CANVAS_KEY_DTYPE = np.dtype([
    ("key_serial", np.uint32), ("slot", np.uint32), ("generation", np.uint32), ("segment", np.uint32), ("start_line", np.uint32),
    ("start_column", np.uint32), ("lines", np.uint32), ("placed", np.uint8), ("reserved", np.uint8, (3,))])
assert CANVAS_KEY_DTYPE.itemsize == 32
_CANVAS_COUNTERS = [(k, np.uint64) for k in (
    "calls", "canvases_begun", "canvases_completed", "segments_begun", "segments_done", "segments_aborted", "lines_placed",
    "lines_clipped", "faults", "bad_segment", "too_large", "duplicate", "overlap", "no_slot", "no_placement")]
# xrit_canvas_counters
CANVAS_STATS_DTYPE = np.dtype(_CANVAS_COUNTERS)
assert CANVAS_STATS_DTYPE.itemsize == 120
# xrit_canvas_summary: a call's counts and the handle's counters after it
CANVAS_SUMMARY_DTYPE = np.dtype([(k, np.uint64) for k in ("placed", "call_lines_placed", "call_lines_clipped", "call_faults", "completed")] +
                                _CANVAS_COUNTERS + [("overflow", np.uint32), ("reserved", np.uint32)])
assert CANVAS_SUMMARY_DTYPE.itemsize == 168


class ImageCanvas(_Handle):
    """A pool of `slots` image canvases of slot_bytes each in device memory.  A call takes what FileAssembler.process and
    ImageDecoder.process on it returned and places every decoded line into the canvas of the image its segment file
    belongs to (the segment identification record, type 128, says where); which canvases are complete is in the slot
    table it returns.  The host reads a finished canvas and releases its slot."""
    _destroy = "xrit_canvas_destroy"

    def __init__(self, slots=8, slot_bytes=1 << 20, device=0):
        super().__init__()
        self.slots, self.slot_bytes = int(slots), int(slot_bytes)
        _check(lib().xrit_canvas_create(C.byref(self._h), device, self.slots, self.slot_bytes))

    def process(self, files_out, images_out):
        """files_out: (bytes, pieces, files, summary) as FileAssembler.process returned them; images_out: (bytes, lines,
        image_files, summary) as ImageDecoder.process returned them on those.  -> (canvas_files CANVAS_FILE_DTYPE, one per
        record of `files`; the slot table after the call, CANVAS_SLOT_DTYPE; summary, a CANVAS_SUMMARY_DTYPE record).
        A summary with overflow != 0, or with counts beyond the arrays' lengths, is refused: XritError -1, `partial`
        with the summary (overflow 2) alone, the state unchanged."""
        data = np.ascontiguousarray(files_out[0], np.uint8).reshape(-1)
        pieces = np.ascontiguousarray(files_out[1], FILE_PIECE_DTYPE).reshape(-1)
        files = np.ascontiguousarray(files_out[2], FILE_RECORD_DTYPE).reshape(-1)
        fsum = np.ascontiguousarray(np.asarray(files_out[3], FILES_SUMMARY_DTYPE).reshape(1))
        img = np.ascontiguousarray(images_out[0], np.uint8).reshape(-1)
        lines = np.ascontiguousarray(images_out[1], IMAGE_LINE_DTYPE).reshape(-1)
        ifiles = np.ascontiguousarray(images_out[2], IMAGE_FILE_DTYPE).reshape(-1)
        isum = np.ascontiguousarray(np.asarray(images_out[3], IMAGES_SUMMARY_DTYPE).reshape(1))
        if len(ifiles) != len(files):
            raise ValueError("one image file per files record")
        cfiles = np.zeros(max(len(files), 1), CANVAS_FILE_DTYPE)
        slots = np.zeros(self.slots, CANVAS_SLOT_DTYPE)
        summary = np.zeros(1, CANVAS_SUMMARY_DTYPE)
        rc = lib().xrit_canvas_process(self._h, _p(data), len(data), _p(pieces), len(pieces), _p(files), len(files), _p(fsum), _p(img),
                                       len(img), _p(lines), len(lines), _p(ifiles), _p(isum), _p(cfiles), _p(slots), _p(summary))
        if rc != 0:
            err = XritError(rc, lib().xrit_last_error().decode("utf-8", "replace"))
            if int(summary[0]["overflow"]) == 2:
                err.partial = (summary[0],)
            raise err
        return cfiles[:len(files)].copy(), slots, summary[0]

    def process_device(self, d_bytes_ptr, n_bytes, d_pieces_ptr, max_pieces_in, d_files_ptr, max_files_in, d_files_summary_ptr,
                       d_image_bytes_ptr, n_image_bytes, d_lines_ptr, max_lines_in, d_image_files_ptr, d_images_summary_ptr,
                       d_canvas_files_ptr, d_slots_ptr, d_summary_ptr, stream=None):
        """Device pointers as FileAssembler.process_device and ImageDecoder.process_device wrote them; canvas files
        max_files_in x 32, slots self.slots x 136, summary 168 bytes.  Asynchronous on stream; may be queued behind
        ImageDecoder.process_device: the counts are read from the two summaries on the device."""
        _check(lib().xrit_canvas_process_device(
            self._h, C.c_void_p(d_bytes_ptr), n_bytes, C.c_void_p(d_pieces_ptr), max_pieces_in, C.c_void_p(d_files_ptr), max_files_in,
            C.c_void_p(d_files_summary_ptr), C.c_void_p(d_image_bytes_ptr), n_image_bytes, C.c_void_p(d_lines_ptr), max_lines_in,
            C.c_void_p(d_image_files_ptr), C.c_void_p(d_images_summary_ptr), C.c_void_p(d_canvas_files_ptr), C.c_void_p(d_slots_ptr),
            C.c_void_p(d_summary_ptr), C.c_void_p(stream) if stream else None))

    def read(self, slot):
        """(the slot's record, its pitch x max_row bytes as a uint8 array (max_row, pitch)) after the last call."""
        info = np.zeros(1, CANVAS_SLOT_DTYPE)
        buf = np.zeros(self.slot_bytes, np.uint8)
        _check(lib().xrit_canvas_read(self._h, slot, _p(buf), len(buf), _p(info)))
        rows, pitch = int(info[0]["max_row"]), int(info[0]["pitch"])
        return info[0], buf[:rows * pitch].reshape(rows, pitch).copy()

    def image(self, slot):
        """(the slot's record, its canvas as samples (max_row, max_column), uint8 or uint16)."""
        info, raw = self.read(slot)
        if int(info["bits"]) <= 8:
            return info, raw[:, :int(info["max_column"])].copy()
        return info, np.ascontiguousarray(raw[:, :2 * int(info["max_column"])]).view("<u2").copy()

    def read_device(self, slot, d_out_ptr, n_bytes, stream=None):
        """The first n_bytes of the slot's pixels to device memory, asynchronous on stream."""
        _check(lib().xrit_canvas_read_device(self._h, slot, C.c_void_p(d_out_ptr), n_bytes, C.c_void_p(stream) if stream else None))

    def segments(self, slot):
        """The slot's 64 segments (CANVAS_SEGMENT_DTYPE; entry segment - 1) after the last call."""
        out = np.zeros(64, CANVAS_SEGMENT_DTYPE)
        _check(lib().xrit_canvas_segments(self._h, slot, _p(out)))
        return out

    def key(self, vcid, apid):
        """What (vcid, apid) carries after the last call (a CANVAS_KEY_DTYPE scalar record); waits for that call."""
        out = np.zeros(1, CANVAS_KEY_DTYPE)
        _check(lib().xrit_canvas_key(self._h, vcid, apid, _p(out)))
        return out[0]

    def stats(self):
        """The counters after the last call (a CANVAS_STATS_DTYPE scalar record); waits for that call."""
        out = np.zeros(1, CANVAS_STATS_DTYPE)
        _check(lib().xrit_canvas_stats(self._h, _p(out)))
        return out[0]

    def release(self, slot):
        """The slot free again, all zero, its generation one more; queued behind the last call."""
        _check(lib().xrit_canvas_release(self._h, slot))

    def reset(self):
        """Every slot free, every key without placement, counters and pixels zero."""
        _check(lib().xrit_canvas_reset(self._h))

    def pixels_device(self, slot):
        """The device address of the slot's pixels, for a stage that reads a canvas in place (ImageProduct.process_device);
        the caller orders what reads them behind the last call."""
        out = C.c_void_p()
        _check(lib().xrit_canvas_pixels_device(self._h, slot, C.byref(out)))
        return int(out.value)


# ---- image products ------------------------------------------------------------------------------
TONE_LINEAR, TONE_TABLE, TONE_EQUALISE, TONE_STRETCH = 0, 1, 2, 3
PRODUCT_TONES = ("linear", "table", "equalise", "stretch")
PRODUCT_MAX_FACTOR = 64
# xrit_product_image with its pointer as an integer, xrit_product_params, xrit_product_summary
PRODUCT_IMAGE_DTYPE = np.dtype([("d_pixels", np.uint64), ("columns", np.uint32), ("rows", np.uint32), ("pitch", np.uint32), ("bits", np.uint32)])
assert PRODUCT_IMAGE_DTYPE.itemsize == 24
PRODUCT_PARAMS_DTYPE = np.dtype([("tone", np.uint32), ("p_lo", np.uint32), ("p_hi", np.uint32), ("factor", np.uint32)])
assert PRODUCT_PARAMS_DTYPE.itemsize == 16
PRODUCT_SUMMARY_DTYPE = np.dtype([("total", np.uint64), ("zeros", np.uint64), ("out_of_range", np.uint64)] +
                                 [(k, np.uint32) for k in ("min_nz", "max_nz", "lo", "hi", "fallback", "tone", "tone_columns", "tone_rows",
                                                           "small_columns", "small_rows")])
assert PRODUCT_SUMMARY_DTYPE.itemsize == 64


def _tone_code(tone):
    return PRODUCT_TONES.index(tone) if isinstance(tone, str) else int(tone)


def _product_args(pixels_ptr, columns, rows, pitch, bits, tone, p_lo, p_hi, factor):
    image = np.zeros(1, PRODUCT_IMAGE_DTYPE)
    image[0] = (pixels_ptr, columns, rows, pitch, bits)
    params = np.zeros(1, PRODUCT_PARAMS_DTYPE)
    params[0] = (_tone_code(tone), p_lo, p_hi, factor)
    return image, params


class ImageProduct(_Handle):
    """What is shown of an image, made on the device: the histogram, a tone table from it (linear, the caller's, equalised,
    or stretched between two percentiles), the toned 8-bit image, a thumbnail that leaves pixels without data (value 0)
    out of its means, and the false-colour composite of two toned images through the caller's 256 x 256 x 3 table.  The
    handle owns scratch only; tests/product_spec.py is the specification."""
    _destroy = "xrit_product_destroy"

    def __init__(self, device=0):
        super().__init__()
        _check(lib().xrit_product_create(C.byref(self._h), device))

    def process(self, image, bits, tone="equalise", p_lo=0, p_hi=10000, factor=0, table=None, outputs=("hist", "lut", "tone", "small")):
        """image: 2-D, uint8 for bits <= 8, uint16 above (its row stride is taken as the pitch).  -> dict with a
        PRODUCT_SUMMARY_DTYPE record under "summary" and, of `outputs`, "hist" (uint32, 2^bits), "lut" (uint8, 2^bits),
        "tone" (uint8, rows x columns) and, for factor > 0, "small"."""
        image = np.asarray(image)
        if image.ndim != 2 or image.dtype != (np.uint8 if bits <= 8 else np.uint16) or image.strides[1] != image.itemsize or image.strides[0] < 0:
            raise ValueError("a 2-D image of uint8 (bits <= 8) or uint16 samples, contiguous along its rows")
        rows, columns = image.shape
        return self._to_host(lib().xrit_product_process, image.ctypes.data, columns, rows,
                             image.strides[0] if rows > 1 else columns * image.itemsize, bits, tone, p_lo, p_hi, factor, table, outputs)

    def process_resident(self, d_pixels_ptr, columns, rows, pitch, bits, tone="equalise", p_lo=0, p_hi=10000, factor=0, table=None,
                         outputs=("hist", "lut", "tone", "small")):
        """As process, on an image that lies in device memory (ImageCanvas.pixels_device, once the canvas's last call has
        finished): nothing is uploaded, only `outputs` are downloaded."""
        return self._to_host(lib().xrit_product_process_resident, d_pixels_ptr, columns, rows, pitch, bits, tone, p_lo, p_hi, factor, table,
                             outputs)

    def _to_host(self, fn, pixels_ptr, columns, rows, pitch, bits, tone, p_lo, p_hi, factor, table, outputs):
        img, params = _product_args(pixels_ptr, columns, rows, pitch, bits, tone, p_lo, p_hi, factor)
        tab = None if table is None else np.ascontiguousarray(table, np.uint8).reshape(-1)
        if tab is not None and len(tab) != 1 << bits:
            raise ValueError("a table of 2^bits bytes")
        out = {}
        if "hist" in outputs:
            out["hist"] = np.zeros(1 << bits, np.uint32)
        if "lut" in outputs:
            out["lut"] = np.zeros(1 << bits, np.uint8)
        if "tone" in outputs:
            out["tone"] = np.zeros((rows, columns), np.uint8)
        if "small" in outputs and factor:
            out["small"] = np.zeros(((rows + factor - 1) // factor, (columns + factor - 1) // factor), np.uint8)
        summary = np.zeros(1, PRODUCT_SUMMARY_DTYPE)
        ptr = lambda k: _p(out[k]) if k in out else None
        _check(fn(self._h, _p(img), _p(params), None if tab is None else _p(tab), ptr("hist"), ptr("lut"), ptr("tone"), ptr("small"),
                  _p(summary)))
        out["summary"] = summary[0]
        return out

    def process_device(self, d_pixels_ptr, columns, rows, pitch, bits, d_summary_ptr, tone="equalise", p_lo=0, p_hi=10000, factor=0,
                       d_table_in_ptr=None, d_hist_ptr=None, d_lut_ptr=None, d_tone_ptr=None, d_small_ptr=None, stream=None):
        """Device pointers; the outputs that are None are not written (the summary always is, 64 bytes).  Asynchronous on
        stream, no host synchronisation: may be queued behind ImageCanvas.process_device on a slot's pixels_device()."""
        img, params = _product_args(d_pixels_ptr, columns, rows, pitch, bits, tone, p_lo, p_hi, factor)
        v = lambda x: C.c_void_p(x) if x else None
        _check(lib().xrit_product_process_device(self._h, _p(img), _p(params), v(d_table_in_ptr), v(d_hist_ptr), v(d_lut_ptr), v(d_tone_ptr),
                                                 v(d_small_ptr), v(d_summary_ptr), v(stream)))

    def outputs_device(self):
        """(d_tone, d_small): where the last process / process_resident left the toned image and the thumbnail in device
        memory (None for one it did not make), for a stage that goes on with them there (JpegEncoder.encode_resident)."""
        tone, small = C.c_void_p(), C.c_void_p()
        _check(lib().xrit_product_outputs_device(self._h, C.byref(tone), C.byref(small)))
        return tone.value, small.value

    def composite(self, a, b, table):
        """a, b: toned 8-bit images of one shape; table: 256 * 256 * 3 bytes -> uint8 (rows, columns, 3)."""
        a, b = np.asarray(a), np.asarray(b)
        if a.ndim != 2 or a.shape != b.shape or a.dtype != np.uint8 or b.dtype != np.uint8 or a.strides[1] != 1 or b.strides[1] != 1:
            raise ValueError("two 2-D uint8 images of one shape, contiguous along their rows")
        tab = np.ascontiguousarray(table, np.uint8).reshape(-1)
        if len(tab) != 256 * 256 * 3:
            raise ValueError("a table of 256 * 256 * 3 bytes")
        rows, columns = a.shape
        rgb = np.zeros((rows, columns, 3), np.uint8)
        pitch = lambda x: x.strides[0] if rows > 1 else columns
        _check(lib().xrit_product_composite(self._h, _p(a), pitch(a), _p(b), pitch(b), columns, rows, _p(tab), _p(rgb)))
        return rgb

    def composite_device(self, d_a_ptr, pitch_a, d_b_ptr, pitch_b, columns, rows, d_table_ptr, d_rgb_ptr, stream=None):
        """Device pointers; rgb rows x columns x 3 bytes.  Asynchronous on stream."""
        v = lambda x: C.c_void_p(x) if x else None
        _check(lib().xrit_product_composite_device(self._h, v(d_a_ptr), pitch_a, v(d_b_ptr), pitch_b, columns, rows, v(d_table_ptr),
                                                   v(d_rgb_ptr), v(stream)))

    def reset(self):
        """Waits for the last call; there is no state."""
        _check(lib().xrit_product_reset(self._h))


# ---- image projection ---------------------------------------------------------------------------
GEO_EQUIRECT, GEO_MERCATOR = 0, 1
GEO_NEAREST, GEO_BILINEAR = 0, 1
GEO_KINDS = ("equirect", "mercator")
GEO_MODES = ("nearest", "bilinear")
GEO_MAX_DIM = 16384
GEO_OFF = -(1 << 31)
# xrit_geo_nav, xrit_geo_grid, xrit_geo_point, xrit_geo_summary
GEO_NAV_DTYPE = np.dtype([("cfac", np.int32), ("lfac", np.int32), ("coff", np.int32), ("loff", np.int32), ("origin", np.int32),
                          ("reserved", np.int32), ("sub_lon_deg", np.float64)])
assert GEO_NAV_DTYPE.itemsize == 32
GEO_GRID_DTYPE = np.dtype([("kind", np.uint32), ("columns", np.uint32), ("rows", np.uint32), ("reserved", np.uint32), ("lon0_deg", np.float64),
                           ("lat0_deg", np.float64), ("step_lon_deg", np.float64), ("step_lat_deg", np.float64)])
assert GEO_GRID_DTYPE.itemsize == 48
GEO_POINT_DTYPE = np.dtype([("qx", np.int32), ("qy", np.int32)])
assert GEO_POINT_DTYPE.itemsize == 8
GEO_SUMMARY_DTYPE = np.dtype([(k, np.uint64) for k in ("total", "off_disc", "outside", "no_data", "written")] +
                             [(k, np.uint32) for k in ("columns", "rows", "width", "mode")])
assert GEO_SUMMARY_DTYPE.itemsize == 56


def _geo_mode(mode):
    return GEO_MODES.index(mode) if isinstance(mode, str) else int(mode)


def geo_nav(cfac, lfac, coff, loff, origin=1, sub_lon_deg=0.0):
    """One xrit_geo_nav record (a GEO_NAV_DTYPE array of one element)."""
    nav = np.zeros(1, GEO_NAV_DTYPE)
    nav[0] = (cfac, lfac, coff, loff, origin, 0, sub_lon_deg)
    return nav


def _geo_nav_arg(nav):
    if isinstance(nav, dict):
        return geo_nav(nav["cfac"], nav["lfac"], nav["coff"], nav["loff"], nav.get("origin", 1), nav.get("sub_lon", nav.get("sub_lon_deg", 0.0)))
    return np.ascontiguousarray(np.asarray(nav, GEO_NAV_DTYPE).reshape(1))


def _geo_grid_arg(kind, columns, rows, lon0_deg, lat0_deg, step_lon_deg, step_lat_deg):
    grid = np.zeros(1, GEO_GRID_DTYPE)
    grid[0] = (GEO_KINDS.index(kind) if isinstance(kind, str) else int(kind), columns, rows, 0, lon0_deg, lat0_deg, step_lon_deg, step_lat_deg)
    return grid


def geo_grid_tables(kind, columns, rows, lon0_deg, lat0_deg, step_lon_deg, step_lat_deg, sub_lon_deg):
    """The library's tables of a grid, made on the host (no device): (A, B of `rows` float64, C, S of `columns`)."""
    grid = _geo_grid_arg(kind, columns, rows, lon0_deg, lat0_deg, step_lon_deg, step_lat_deg)
    n_r, n_c = max(int(rows), 0), max(int(columns), 0)
    A, B, Cc, S = np.zeros(n_r), np.zeros(n_r), np.zeros(n_c), np.zeros(n_c)
    _check(lib().xrit_geo_grid_tables(_p(grid), float(sub_lon_deg), _p(A), _p(B), _p(Cc), _p(S)))
    return A, B, Cc, S


def geo_parse_navigation(header):
    """The navigation record (type 2) of a file's header bytes -> a GEO_NAV_DTYPE record; XritError -1 without one."""
    b = np.frombuffer(bytes(header), np.uint8)
    nav = np.zeros(1, GEO_NAV_DTYPE)
    _check(lib().xrit_geo_parse_navigation(_p(b) if len(b) else None, len(b), _p(nav)))
    return nav[0]


def geo_pixel_to_lonlat(nav, column, line):
    """The inverse of the map: (lon_deg, lat_deg) of what (column, line) looks at, None for space."""
    nav = _geo_nav_arg(nav)
    lon, lat = C.c_double(), C.c_double()
    rc = lib().xrit_geo_pixel_to_lonlat(_p(nav), float(column), float(line), C.byref(lon), C.byref(lat))
    if rc == 1:
        return None
    _check(rc)
    return lon.value, lat.value


class ImageProjector(_Handle):
    """An image in the instrument's scan geometry resampled onto a latitude / longitude grid on the device.  The handle
    holds the grid as four tables (set_grid, set_tables); project is the fused call, map + resample the pair for one
    geometry with many channels.  tests/geo_spec.py is the specification."""
    _destroy = "xrit_geo_destroy"

    def __init__(self, device=0):
        super().__init__()
        _check(lib().xrit_geo_create(C.byref(self._h), device))
        self.columns = self.rows = 0

    def set_grid(self, kind, columns, rows, lon0_deg, lat0_deg, step_lon_deg, step_lat_deg, sub_lon_deg):
        grid = _geo_grid_arg(kind, columns, rows, lon0_deg, lat0_deg, step_lon_deg, step_lat_deg)
        _check(lib().xrit_geo_set_grid(self._h, _p(grid), float(sub_lon_deg)))
        self.columns, self.rows = int(columns), int(rows)

    def set_tables(self, A, B, Cc, S):
        A, B, Cc, S = (np.ascontiguousarray(x, np.float64).reshape(-1) for x in (A, B, Cc, S))
        if len(A) != len(B) or len(Cc) != len(S):
            raise ValueError("A and B per row, C and S per column")
        _check(lib().xrit_geo_set_tables(self._h, len(Cc), len(A), _p(A), _p(B), _p(Cc), _p(S)))
        self.columns, self.rows = len(Cc), len(A)

    def tables(self):
        """The tables in effect, read back from the device: (A, B, C, S)."""
        c, r = C.c_uint32(), C.c_uint32()
        _check(lib().xrit_geo_tables(self._h, C.byref(c), C.byref(r), None, None, None, None))
        A, B, Cc, S = np.zeros(r.value), np.zeros(r.value), np.zeros(c.value), np.zeros(c.value)
        _check(lib().xrit_geo_tables(self._h, None, None, _p(A), _p(B), _p(Cc), _p(S)))
        return A, B, Cc, S

    def _image(self, pixels_ptr, columns, rows, pitch, bits):
        image = np.zeros(1, PRODUCT_IMAGE_DTYPE)
        image[0] = (pixels_ptr or 0, columns, rows, pitch, bits)
        return image

    def map_device(self, nav, d_map_ptr, stream=None):
        """rows x columns GEO_POINT_DTYPE entries to device memory.  Asynchronous on stream."""
        v = lambda x: C.c_void_p(x) if x else None
        _check(lib().xrit_geo_map_device(self._h, _p(_geo_nav_arg(nav)), v(d_map_ptr), v(stream)))

    def resample_device(self, d_pixels_ptr, columns, rows, pitch, bits, d_map_ptr, mode, d_out_ptr, out_pitch, d_summary_ptr, stream=None):
        v = lambda x: C.c_void_p(x) if x else None
        _check(lib().xrit_geo_resample_device(self._h, _p(self._image(d_pixels_ptr, columns, rows, pitch, bits)), v(d_map_ptr), _geo_mode(mode),
                                              v(d_out_ptr), out_pitch, v(d_summary_ptr), v(stream)))

    def project_device(self, nav, d_pixels_ptr, columns, rows, pitch, bits, mode, d_out_ptr, out_pitch, d_summary_ptr, stream=None):
        """Fused; may be queued behind ImageCanvas.process_device on a slot's pixels_device().  Asynchronous on stream."""
        v = lambda x: C.c_void_p(x) if x else None
        _check(lib().xrit_geo_project_device(self._h, _p(_geo_nav_arg(nav)), _p(self._image(d_pixels_ptr, columns, rows, pitch, bits)),
                                             _geo_mode(mode), v(d_out_ptr), out_pitch, v(d_summary_ptr), v(stream)))

    def _to_host(self, fn, nav, pixels_ptr, columns, rows, pitch, bits, mode):
        out = np.zeros((self.rows, self.columns), np.uint8 if bits <= 8 else np.uint16)
        summary = np.zeros(1, GEO_SUMMARY_DTYPE)
        _check(fn(self._h, _p(_geo_nav_arg(nav)), _p(self._image(pixels_ptr, columns, rows, pitch, bits)), _geo_mode(mode), _p(out),
                  self.columns * out.itemsize, _p(summary)))
        return out, summary[0]

    def project(self, nav, image, bits, mode="bilinear"):
        """image: 2-D, uint8 for bits <= 8, uint16 above (its row stride is the pitch) -> (the projected image, a
        GEO_SUMMARY_DTYPE record)."""
        image = np.asarray(image)
        if image.ndim != 2 or image.dtype != (np.uint8 if bits <= 8 else np.uint16) or image.strides[1] != image.itemsize or image.strides[0] < 0:
            raise ValueError("a 2-D image of uint8 (bits <= 8) or uint16 samples, contiguous along its rows")
        rows, columns = image.shape
        return self._to_host(lib().xrit_geo_project, nav, image.ctypes.data, columns, rows,
                             image.strides[0] if rows > 1 else columns * image.itemsize, bits, mode)

    def project_resident(self, nav, d_pixels_ptr, columns, rows, pitch, bits, mode="bilinear"):
        """As project, on an image that lies in device memory (ImageCanvas.pixels_device, once the canvas's last call has
        finished)."""
        return self._to_host(lib().xrit_geo_project_resident, nav, d_pixels_ptr, columns, rows, pitch, bits, mode)

    def reset(self):
        """Waits for the last call; the tables stay."""
        _check(lib().xrit_geo_reset(self._h))


# ---- map overlay ----------------------------------------------------------------------------------
OVERLAY_BREAK = -(1 << 31)
OVERLAY_LIMIT = 1 << 29
OVERLAY_MAX_DIM = 16384
OVERLAY_MAX_WIDTH = 8
OVERLAY_LAYERS = 8
OVERLAY_MAX_VERTICES = 1 << 26
# xrit_overlay_style, xrit_overlay_draw_summary, xrit_overlay_blend_summary
OVERLAY_STYLE_DTYPE = np.dtype([("r", np.uint8), ("g", np.uint8), ("b", np.uint8), ("alpha", np.uint8)])
assert OVERLAY_STYLE_DTYPE.itemsize == 4
OVERLAY_DRAW_SUMMARY_DTYPE = np.dtype([(k, np.uint64) for k in ("vertices", "segments", "hidden", "jumps", "outside", "drawn", "steps")] +
                                      [(k, np.uint32) for k in ("layer", "width")])
assert OVERLAY_DRAW_SUMMARY_DTYPE.itemsize == 64
OVERLAY_BLEND_SUMMARY_DTYPE = np.dtype([("pixels", np.uint64), ("covered", np.uint64), ("by_layer", np.uint64, (8,))] +
                                       [(k, np.uint32) for k in ("columns", "rows", "components_in", "components_out")])
assert OVERLAY_BLEND_SUMMARY_DTYPE.itemsize == 96


def overlay_styles(styles):
    """8 x (r, g, b, alpha) -> an OVERLAY_STYLE_DTYPE array of 8."""
    if isinstance(styles, np.ndarray) and styles.dtype == OVERLAY_STYLE_DTYPE and styles.shape == (OVERLAY_LAYERS,):
        return np.ascontiguousarray(styles)
    a = np.asarray(styles, np.int64).reshape(OVERLAY_LAYERS, 4)
    if (a < 0).any() or (a > 255).any():
        raise ValueError("r, g, b and alpha are bytes")
    return np.ascontiguousarray(a.astype(np.uint8)).view(OVERLAY_STYLE_DTYPE).reshape(OVERLAY_LAYERS)


def _overlay_points_arg(points):
    if isinstance(points, np.ndarray) and points.dtype == GEO_POINT_DTYPE:
        return np.ascontiguousarray(points.reshape(-1))
    a = np.ascontiguousarray(np.asarray(points, np.int64).reshape(-1, 2).astype(np.int32))
    return a.view(GEO_POINT_DTYPE).reshape(-1)


def _lonlat(lon_deg, lat_deg):
    lon, lat = np.ascontiguousarray(lon_deg, np.float64).reshape(-1), np.ascontiguousarray(lat_deg, np.float64).reshape(-1)
    if len(lon) != len(lat):
        raise ValueError("a latitude per longitude")
    return lon, lat


def overlay_quads(lon_deg, lat_deg, sub_lon_deg):
    """The quads {A, B, C, S} of vertices given in degrees, made on the host (no device): (n, 4) float64; NaN: a NaN quad."""
    lon, lat = _lonlat(lon_deg, lat_deg)
    quads = np.zeros((len(lon), 4))
    _check(lib().xrit_overlay_quads(_p(lon), _p(lat), len(lon), float(sub_lon_deg), _p(quads)))
    return quads


def overlay_grid_points(kind, columns, rows, lon0_deg, lat0_deg, step_lon_deg, step_lat_deg, lon_deg, lat_deg):
    """The positions on a grid in 1/256 pixel (no device): GEO_POINT_DTYPE; NaN or out of range: a break."""
    lon, lat = _lonlat(lon_deg, lat_deg)
    grid = _geo_grid_arg(kind, columns, rows, lon0_deg, lat0_deg, step_lon_deg, step_lat_deg)
    points = np.zeros(len(lon), GEO_POINT_DTYPE)
    _check(lib().xrit_overlay_grid_points(_p(grid), _p(lon), _p(lat), len(lon), _p(points)))
    return points


def _overlay_sized(call):
    """A host helper with a capacity: asked for the count first, then for the vertices."""
    n = C.c_size_t()
    rc = call(None, None, 0, n)
    if rc not in (0, -5):
        _check(rc)
    lon, lat = np.zeros(n.value), np.zeros(n.value)
    _check(call(_p(lon), _p(lat), n.value, n))
    return lon, lat


def overlay_densify(lon_deg, lat_deg, max_step_deg):
    """Segments longer than max_step_deg in either coordinate split into equal parts; NaN vertices are breaks and stay."""
    lon, lat = _lonlat(lon_deg, lat_deg)
    return _overlay_sized(lambda a, b, cap, n: lib().xrit_overlay_densify(_p(lon), _p(lat), len(lon), float(max_step_deg), a, b, cap, C.byref(n)))


def overlay_graticule(step_deg, vertex_step_deg):
    """Meridians and parallels every step_deg with a vertex every vertex_step_deg, a NaN break behind each line."""
    return _overlay_sized(lambda a, b, cap, n: lib().xrit_overlay_graticule(float(step_deg), float(vertex_step_deg), a, b, cap, C.byref(n)))


class MapOverlay(_Handle):
    """Polylines (coastlines, borders, a graticule) drawn into a mask of one byte per pixel, bit k for layer k, and the
    mask blended into an 8-bit image, on the device.  form 0: a lane per segment; form 1: a lane per step.  The handle
    owns scratch and the form; tests/overlay_spec.py is the specification."""
    _destroy = "xrit_overlay_destroy"

    def __init__(self, form=1, device=0):
        super().__init__()
        _check(lib().xrit_overlay_create(C.byref(self._h), device))
        self.set_form(form)

    def set_form(self, form):
        _check(lib().xrit_overlay_set_form(self._h, form))

    @staticmethod
    def _image(pixels_ptr, columns, rows, pitch):
        image = np.zeros(1, PRODUCT_IMAGE_DTYPE)
        image[0] = (pixels_ptr or 0, columns, rows, pitch, 8)
        return image

    def map_device(self, nav, d_quads_ptr, n, d_points_ptr, stream=None):
        """n quads of four float64 -> n GEO_POINT_DTYPE entries, both in device memory.  Asynchronous on stream."""
        v = lambda x: C.c_void_p(x) if x else None
        _check(lib().xrit_overlay_map_device(self._h, _p(_geo_nav_arg(nav)), v(d_quads_ptr), n, v(d_points_ptr), v(stream)))

    def draw_device(self, d_points_ptr, n, layer, width, max_jump, d_mask_ptr, columns, rows, mask_pitch, clear, d_summary_ptr, stream=None):
        """Asynchronous on stream; ORs into the mask unless clear."""
        v = lambda x: C.c_void_p(x) if x else None
        _check(lib().xrit_overlay_draw_device(self._h, v(d_points_ptr), n, layer, width, max_jump, v(d_mask_ptr), columns, rows, mask_pitch,
                                              1 if clear else 0, v(d_summary_ptr), v(stream)))

    def blend_device(self, d_pixels_ptr, columns, rows, pitch, components_in, d_mask_ptr, mask_pitch, styles, d_out_ptr, out_pitch,
                     components_out, d_summary_ptr, stream=None):
        """Asynchronous on stream; d_out_ptr may be d_pixels_ptr when components and pitches are equal."""
        v = lambda x: C.c_void_p(x) if x else None
        _check(lib().xrit_overlay_blend_device(self._h, _p(self._image(d_pixels_ptr, columns, rows, pitch)), components_in, v(d_mask_ptr),
                                               mask_pitch, _p(overlay_styles(styles)) if styles is not None else None, v(d_out_ptr), out_pitch,
                                               components_out, v(d_summary_ptr), v(stream)))

    def map(self, nav, quads):
        """quads: (n, 4) float64 -> n GEO_POINT_DTYPE entries."""
        q = np.ascontiguousarray(quads, np.float64).reshape(-1, 4)
        points = np.zeros(len(q), GEO_POINT_DTYPE)
        _check(lib().xrit_overlay_map(self._h, _p(_geo_nav_arg(nav)), _p(q), len(q), _p(points)))
        return points

    def draw(self, points, layer, width, mask, max_jump=0, clear=False):
        """points: GEO_POINT_DTYPE or (n, 2) integers; mask: 2-D uint8, C-contiguous, its row length a multiple of 4 and at
        least `columns` -- drawn into in place.  columns: mask.shape[1] -> the OVERLAY_DRAW_SUMMARY_DTYPE record."""
        return self.draw_into(points, layer, width, mask, mask.shape[1], max_jump, clear)

    def draw_into(self, points, layer, width, mask, columns, max_jump=0, clear=False):
        """As draw, for a mask whose rows are longer than the image's `columns`."""
        if not (isinstance(mask, np.ndarray) and mask.dtype == np.uint8 and mask.ndim == 2 and mask.flags.c_contiguous and mask.flags.writeable):
            raise ValueError("a writeable C-contiguous 2-D uint8 mask")
        pts = _overlay_points_arg(points)
        summary = np.zeros(1, OVERLAY_DRAW_SUMMARY_DTYPE)
        _check(lib().xrit_overlay_draw(self._h, _p(pts) if len(pts) else None, len(pts), layer, width, max_jump, _p(mask), columns, mask.shape[0],
                                       mask.shape[1], 1 if clear else 0, _p(summary)))
        return summary[0]

    def _blend_to_host(self, fn, pixels_ptr, columns, rows, pitch, components_in, mask_ptr, mask_pitch, styles, components_out):
        out = np.zeros((rows, columns) if components_out == 1 else (rows, columns, 3), np.uint8)
        summary = np.zeros(1, OVERLAY_BLEND_SUMMARY_DTYPE)
        _check(fn(self._h, _p(self._image(pixels_ptr, columns, rows, pitch)), components_in, C.c_void_p(mask_ptr), mask_pitch,
                  _p(overlay_styles(styles)), _p(out), columns * components_out, components_out, _p(summary)))
        return out, summary[0]

    def blend(self, image, mask, styles, components_out=3):
        """image: (rows, columns) or (rows, columns, 3) uint8; mask: (rows, columns) uint8 -> (the blended image, an
        OVERLAY_BLEND_SUMMARY_DTYPE record)."""
        image, mask = np.ascontiguousarray(image, np.uint8), np.ascontiguousarray(mask, np.uint8)
        if image.ndim not in (2, 3) or (image.ndim == 3 and image.shape[2] != 3) or mask.shape != image.shape[:2]:
            raise ValueError("an image of one or three interleaved components and a mask of its size")
        rows, columns = mask.shape
        cin = 1 if image.ndim == 2 else 3
        return self._blend_to_host(lib().xrit_overlay_blend, image.ctypes.data, columns, rows, columns * cin, cin, mask.ctypes.data, columns,
                                   styles, components_out)

    def blend_resident(self, d_pixels_ptr, columns, rows, pitch, components_in, d_mask_ptr, mask_pitch, styles, components_out=3):
        """As blend, on an image and a mask that lie in device memory."""
        return self._blend_to_host(lib().xrit_overlay_blend_resident, d_pixels_ptr, columns, rows, pitch, components_in, d_mask_ptr, mask_pitch,
                                   styles, components_out)

    def mask_device(self):
        """Where the last draw / draw_into left the mask in device memory (an int, for blend_resident), None before any."""
        p = C.c_void_p()
        _check(lib().xrit_overlay_mask_device(self._h, C.byref(p)))
        return p.value

    def reset(self):
        """Waits for the last call; there is no state."""
        _check(lib().xrit_overlay_reset(self._h))


# ---- JPEG ---------------------------------------------------------------------------------------
JPEG_MAX_BLOCKS = 1 << 22
# xrit_jpeg_result: what an encode leaves for the caller
JPEG_RESULT_DTYPE = np.dtype([("size", np.uint64), ("status", np.uint32), ("restarts", np.uint32)])
assert JPEG_RESULT_DTYPE.itemsize == 16


def jpeg_bound(components, columns, rows, restart=0):
    """The largest file any input of that shape can produce; 0 for a shape the stage refuses.  Plain host code."""
    return int(lib().xrit_jpeg_bound(components, columns, rows, restart))


def jpeg_quality_tables(quality):
    """libjpeg's scaling of the Annex K tables -> uint8 (2, 64), natural order.  Plain host code."""
    t = np.zeros((2, 64), np.uint8)
    _check(lib().xrit_jpeg_quality_tables(quality, _p(t)))
    return t


def jpeg_header(tables, restart, components, columns, rows):
    """SOI .. SOS as the device writes them for these tables ((2, 64), natural order).  Plain host code: no device."""
    t = np.ascontiguousarray(tables, np.uint8).reshape(-1)
    if len(t) != 128:
        raise ValueError("two tables of 64 bytes")
    out, n = np.zeros(1024, np.uint8), _sz()
    _check(lib().xrit_jpeg_header_for(_p(t), restart, components, columns, rows, _p(out), len(out), C.byref(n)))
    return out[:n.value].tobytes()


class JpegEncoder(_Handle):
    """An 8-bit image in device memory -> a complete baseline JFIF file in device memory, the file libjpeg writes for the
    same pixels: quality 1 .. 100 (libjpeg's scaling of the Annex K tables) or the caller's two tables ((2, 64), natural
    order, entries 1 .. 255); restart in MCUs (0: none).  One component (H x W) or interleaved RGB (H x W x 3), coded
    4:4:4.  The handle owns scratch and the parameters; tests/jpeg_spec.py is the specification."""
    _destroy = "xrit_jpeg_destroy"

    def __init__(self, quality=90, restart=0, tables=None, device=0):
        super().__init__()
        _check(lib().xrit_jpeg_create(C.byref(self._h), device))
        if tables is None:
            self.set_quality(quality, restart)
        else:
            self.set_tables(tables, restart)

    def set_quality(self, quality, restart=0):
        _check(lib().xrit_jpeg_set_quality(self._h, quality, restart))
        self.restart = restart

    def set_tables(self, tables, restart=0):
        t = np.ascontiguousarray(tables, np.uint8).reshape(-1)
        if len(t) != 128:
            raise ValueError("two tables of 64 bytes")
        _check(lib().xrit_jpeg_set_tables(self._h, _p(t), restart))
        self.restart = restart

    def header(self, components, columns, rows):
        """The bytes SOI .. SOS the device will write for that shape.  Host only."""
        out, n = np.zeros(1024, np.uint8), _sz()
        _check(lib().xrit_jpeg_header(self._h, components, columns, rows, _p(out), len(out), C.byref(n)))
        return out[:n.value].tobytes()

    def bound(self, components, columns, rows):
        return jpeg_bound(components, columns, rows, self.restart)

    @staticmethod
    def _image(pixels_ptr, columns, rows, pitch):
        image = np.zeros(1, PRODUCT_IMAGE_DTYPE)
        image[0] = (pixels_ptr or 0, columns, rows, pitch, 8)
        return image

    def _to_host(self, fn, pixels_ptr, columns, rows, pitch, components, cap):
        cap = self.bound(components, columns, rows) if cap is None else cap
        out, result = np.zeros(max(cap, 1), np.uint8), np.zeros(1, JPEG_RESULT_DTYPE)
        _check(fn(self._h, _p(self._image(pixels_ptr, columns, rows, pitch)), components, _p(out), cap, _p(result)))
        return out[:int(result[0]["size"])].tobytes()

    def encode(self, image, cap=None):
        """image: uint8, H x W or H x W x 3, contiguous along its rows (its row stride is the pitch) -> the file's bytes.
        cap: the room for the file (default: the bound); XritError -5 when the file does not fit."""
        image = np.asarray(image)
        if image.dtype != np.uint8 or image.ndim not in (2, 3) or (image.ndim == 3 and image.shape[2] != 3):
            raise ValueError("a uint8 image of shape H x W or H x W x 3")
        rows, columns = image.shape[:2]
        comps = 1 if image.ndim == 2 else 3
        if image.strides[0] < 0 or image.strides[1] != comps or (comps == 3 and image.strides[2] != 1):
            raise ValueError("an image contiguous along its rows")
        return self._to_host(lib().xrit_jpeg_encode, image.ctypes.data, columns, rows, image.strides[0] if rows > 1 else columns * comps,
                             comps, cap)

    def encode_resident(self, d_pixels_ptr, columns, rows, pitch, components, cap=None):
        """As encode, on pixels that lie in device memory: nothing is uploaded, only the file's bytes are downloaded."""
        return self._to_host(lib().xrit_jpeg_encode_resident, d_pixels_ptr, columns, rows, pitch, components, cap)

    def encode_device(self, d_pixels_ptr, columns, rows, pitch, components, d_out_ptr, cap, d_result_ptr, stream=None):
        """Device pointers; the file goes to d_out (at most cap bytes), 16 bytes of JPEG_RESULT_DTYPE to d_result.
        Asynchronous on stream, no host synchronisation: may be queued behind ImageProduct.process_device,
        composite_device and ImageProjector.project_device."""
        v = lambda x: C.c_void_p(x) if x else None
        _check(lib().xrit_jpeg_encode_device(self._h, _p(self._image(d_pixels_ptr, columns, rows, pitch)), components, v(d_out_ptr), cap,
                                             v(d_result_ptr), v(stream)))

    def reset(self):
        """Waits for the last call; the parameters stay."""
        _check(lib().xrit_jpeg_reset(self._h))


# ---- JPEG decoder ---------------------------------------------------------------------------------
(JPEGDEC_OK, JPEGDEC_UNSUPPORTED, JPEGDEC_DAMAGED, JPEGDEC_TOO_LARGE, JPEGDEC_BAD_CODE, JPEGDEC_INDEX, JPEGDEC_SHORT, JPEGDEC_INTERVALS,
 JPEGDEC_RST_ORDER, JPEGDEC_MARKER) = range(10)
JPEGDEC_MAX_BLOCKS = 1 << 22
# xrit_jpegdec_record, xrit_jpegdec_summary, xrit_jpegdec_info
JPEGDEC_RECORD_DTYPE = np.dtype([("offset", np.uint64), ("length", np.uint64), ("columns", np.uint32), ("rows", np.uint32), ("components", np.uint32),
                                 ("restart", np.uint32), ("intervals", np.uint32), ("status", np.uint32), ("reserved", np.uint32, 6)])
JPEGDEC_SUMMARY_DTYPE = np.dtype([("images", np.uint64), ("bytes", np.uint64), ("by_status", np.uint32, 10), ("overflow", np.uint32),
                                  ("reserved", np.uint32)])
JPEGDEC_INFO_DTYPE = np.dtype([("columns", np.uint32), ("rows", np.uint32), ("components", np.uint32), ("restart", np.uint32), ("status", np.uint32),
                               ("scan_offset", np.uint32), ("blocks", np.uint32), ("intervals", np.uint32)])
# the record that names a stream: it begins {uint64 offset; uint32 length}
JPEGDEC_ITEM_DTYPE = np.dtype([("offset", np.uint64), ("length", np.uint32), ("reserved", np.uint32)])
assert JPEGDEC_RECORD_DTYPE.itemsize == 64 and JPEGDEC_SUMMARY_DTYPE.itemsize == 64 and JPEGDEC_INFO_DTYPE.itemsize == 32


def jpegdec_header(data):
    """The header chain of one JPEG stream -> a JPEGDEC_INFO_DTYPE record: geometry and status (0 .. 3).  Plain host code."""
    a = np.frombuffer(bytes(data), np.uint8)
    info = np.zeros(1, JPEGDEC_INFO_DTYPE)
    _check(lib().xrit_jpegdec_header(_p(a) if len(a) else None, len(a), _p(info)))
    return info[0]


class JpegDecoder(_Handle):
    """A batch of baseline JPEG streams -> the pixels libjpeg gives for them, back to back, one JPEGDEC_RECORD_DTYPE per
    stream and a summary.  One component, or three sampled 1 x 1 (YCbCr -> interleaved RGB).  form 0: a lane per restart
    interval; form 1: a wave per interval over subsequences of subsequence_bits.  The handle owns scratch and the form;
    tests/jpegdec_spec.py is the specification."""
    _destroy = "xrit_jpegdec_destroy"

    def __init__(self, form=1, subsequence_bits=0, device=0):
        super().__init__()
        _check(lib().xrit_jpegdec_create(C.byref(self._h), device))
        self.set_form(form, subsequence_bits)

    def set_form(self, form, subsequence_bits=0):
        _check(lib().xrit_jpegdec_set_form(self._h, form, subsequence_bits))

    def decode(self, data, items, cap=None):
        """data: the bytes that hold the streams; items: (offset, length) pairs, or an array whose records begin
        {uint64 offset; uint32 length}.  -> (pixels uint8, records, summary).  cap: the room for the pixels (default: what
        the headers ask for); XritError -5 when an image did not fit (the records and the summary are in the error's
        `records` and `summary`, the prefix that fitted in `pixels`)."""
        a = np.frombuffer(bytes(data), np.uint8) if not isinstance(data, np.ndarray) else np.ascontiguousarray(data, np.uint8)
        if isinstance(items, np.ndarray) and items.dtype.fields:
            rec = np.ascontiguousarray(items)
        else:
            rec = np.zeros(len(items), JPEGDEC_ITEM_DTYPE)
            for i, (offset, length) in enumerate(items):
                rec[i] = (offset, length, 0)
        if cap is None:
            cap = 0
            for r in rec:
                off, n = int(r["offset"]), int(r["length"])
                if off <= len(a) and n <= len(a) - off:
                    info = jpegdec_header(a[off:off + n])
                    if info["status"] == 0:
                        cap += (int(info["columns"]) * int(info["rows"]) * int(info["components"]) + 3) & ~3
        pixels, records, summary = np.zeros(max(cap, 1), np.uint8), np.zeros(len(rec), JPEGDEC_RECORD_DTYPE), np.zeros(1, JPEGDEC_SUMMARY_DTYPE)
        rc = lib().xrit_jpegdec_decode(self._h, _p(a) if len(a) else None, len(a), _p(rec) if len(rec) else None, rec.dtype.itemsize, len(rec),
                                       _p(pixels) if cap else None, cap, _p(records) if len(rec) else None, _p(summary))
        if rc == -5:
            err = XritError(rc, lib().xrit_last_error().decode("utf-8", "replace"))
            err.pixels, err.records, err.summary = pixels[:cap], records, summary[0]
            raise err
        _check(rc)
        return pixels[:min(cap, int(summary[0]["bytes"]))], records, summary[0]

    def decode_device(self, d_bytes_ptr, n_bytes, d_items_ptr, stride, n_items, d_pixels_ptr, cap, d_records_ptr, d_summary_ptr, max_blocks=0,
                      stream=None):
        """Device pointers; asynchronous on stream, no host synchronisation once the scratch has its size: may be queued in
        front of ImageProduct, ImageProjector and JpegEncoder calls that read the pixels in place."""
        v = lambda x: C.c_void_p(x) if x else None
        _check(lib().xrit_jpegdec_decode_device(self._h, v(d_bytes_ptr), n_bytes, v(d_items_ptr), stride, n_items, max_blocks, v(d_pixels_ptr), cap,
                                                v(d_records_ptr), v(d_summary_ptr), v(stream)))

    def rounds(self):
        """The most rounds a tile of 64 subsequences took in the last call (form 1; waits for the call)."""
        n = C.c_uint32()
        _check(lib().xrit_jpegdec_rounds(self._h, C.byref(n)))
        return n.value

    def reset(self):
        """Waits for the last call; the form stays."""
        _check(lib().xrit_jpegdec_reset(self._h))


# ---- carrier acquisition -------------------------------------------------------------------------
ACQUIRE_OK, ACQUIRE_TOO_SHORT, ACQUIRE_WEAK = 0, 1, 2
# xrit_acquire_params
ACQUIRE_PARAMS_DTYPE = np.dtype([("sample_rate", np.float64), ("pre_sum", np.uint32), ("segments", np.uint32), ("min_ratio", np.float64)])
assert ACQUIRE_PARAMS_DTYPE.itemsize == 24
# xrit_acquire_estimate_record: what an estimate writes
ACQUIRE_RECORD_DTYPE = np.dtype([
    ("status", np.uint32), ("k0", np.uint32), ("segments", np.uint32), ("reserved0", np.uint32), ("ratio", np.float64), ("nu", np.float64),
    ("hz", np.float64), ("inc", np.int64), ("applied", np.uint32), ("reserved", np.uint32, (3,))])
assert ACQUIRE_RECORD_DTYPE.itemsize == 64
# xrit_acquire_state: what the handle carries
ACQUIRE_STATE_DTYPE = np.dtype([("acc", np.uint64), ("inc", np.int64), ("samples_mixed", np.uint64), ("estimates", np.uint64),
                                ("applied", np.uint64)])
assert ACQUIRE_STATE_DTYPE.itemsize == 40
_SAMPLE_DTYPES = {SAMPLE_FLOATIQ: (np.complex64, 1), SAMPLE_S16IQ: (np.int16, 2), SAMPLE_S8IQ: (np.int8, 2)}


class CarrierAcquirer(_Handle):
    """A stage in front of the chain: `estimate` finds the carrier offset of a block of raw samples from the spectral
    line of the squared signal (unambiguous for |f| < sample_rate / (4 * pre_sum)), `mix` takes the state's frequency
    out with an oscillator whose 64-bit phase lives in device memory, so a stream may be cut into calls anywhere.  The
    output is cf32 for the chain's SAMPLE_FLOATIQ.  0 for pre_sum, segments or min_ratio selects the default."""
    _destroy = "xrit_acquire_destroy"

    def __init__(self, sample_rate, pre_sum=0, segments=0, min_ratio=0.0, device=0):
        super().__init__()
        par = np.zeros(1, ACQUIRE_PARAMS_DTYPE)
        par[0] = (sample_rate, pre_sum, segments, min_ratio)
        _check(lib().xrit_acquire_create(C.byref(self._h), _p(par), device))

    @staticmethod
    def _samples(samples, sample_type):
        if sample_type not in _SAMPLE_DTYPES:
            raise XritError(-1, "acquire: FLOATIQ, S16IQ and S8IQ are taken")
        dtype, per = _SAMPLE_DTYPES[sample_type]
        a = np.ascontiguousarray(samples, dtype).reshape(-1)
        return a, len(a) // per

    def estimate(self, samples, sample_type=SAMPLE_FLOATIQ, apply=False):
        """-> an ACQUIRE_RECORD_DTYPE scalar record.  apply: a result with status OK becomes the state's frequency."""
        a, n = self._samples(samples, sample_type)
        rec = np.zeros(1, ACQUIRE_RECORD_DTYPE)
        _check(lib().xrit_acquire_estimate(self._h, _p(a), n, sample_type, int(bool(apply)), _p(rec)))
        return rec[0]

    def mix(self, samples, sample_type=SAMPLE_FLOATIQ):
        """-> the samples derotated by the state's oscillator, complex64; the phase carries on into the next call."""
        a, n = self._samples(samples, sample_type)
        out = np.zeros(n, np.complex64)
        _check(lib().xrit_acquire_mix(self._h, _p(a), n, sample_type, _p(out)))
        return out

    def estimate_device(self, d_samples_ptr, n_complex, sample_type, apply, d_record_ptr, stream=None):
        """Device pointers; the 64-byte record is always written.  Asynchronous on stream."""
        _check(lib().xrit_acquire_estimate_device(self._h, C.c_void_p(d_samples_ptr), n_complex, sample_type, int(bool(apply)),
                                                  C.c_void_p(d_record_ptr), C.c_void_p(stream) if stream else None))

    def mix_device(self, d_samples_ptr, n_complex, sample_type, d_out_ptr, stream=None):
        """Device pointers; d_out takes n_complex cf32 and may be d_samples for SAMPLE_FLOATIQ.  Asynchronous on stream:
        it may be queued behind estimate_device and in front of Demodulator.process_device."""
        _check(lib().xrit_acquire_mix_device(self._h, C.c_void_p(d_samples_ptr), n_complex, sample_type, C.c_void_p(d_out_ptr),
                                             C.c_void_p(stream) if stream else None))

    def set_frequency(self, hz):
        """The oscillator's frequency from now on (|hz| < sample_rate / 2); its phase goes on from where it is."""
        _check(lib().xrit_acquire_set_frequency(self._h, float(hz)))

    def state(self):
        """acc, inc and the counters after the last call (an ACQUIRE_STATE_DTYPE scalar record); waits for that call."""
        out = np.zeros(1, ACQUIRE_STATE_DTYPE)
        _check(lib().xrit_acquire_get_state(self._h, _p(out)))
        return out[0]

    def reset(self):
        """Phase, frequency and counters zero."""
        _check(lib().xrit_acquire_reset(self._h))


# ---- link monitor ----------------------------------------------------------------------------------
SYMBOL_F32, SYMBOL_I8 = 0, 1
MONITOR_NO_SIGNAL, MONITOR_NO_NOISE = 1, 2
# xrit_monitor_block: one block of symbols, sums on the integer lattice
MONITOR_BLOCK_DTYPE = np.dtype([
    ("first", np.uint64), ("n", np.uint32), ("flips", np.uint32), ("s1", np.uint64), ("s2", np.uint64), ("s4", np.uint64), ("sum", np.int64),
    ("sat", np.uint32), ("clamped", np.uint32), ("bad", np.uint32), ("neg", np.uint32)])
assert MONITOR_BLOCK_DTYPE.itemsize == 64
# xrit_monitor_summary: what a push leaves for the caller
MONITOR_SUMMARY_DTYPE = np.dtype([("rows", np.uint64), ("open_n", np.uint64), ("symbols_total", np.uint64), ("blocks_total", np.uint64)])
assert MONITOR_SUMMARY_DTYPE.itemsize == 32
# xrit_monitor_state: what the handle carries
MONITOR_STATE_DTYPE = np.dtype([("open", MONITOR_BLOCK_DTYPE), ("symbols_total", np.uint64), ("blocks_total", np.uint64), ("calls", np.uint64),
                                ("last_neg", np.uint32), ("have_last", np.uint32), ("hist", np.uint64, (256,))])
assert MONITOR_STATE_DTYPE.itemsize == 2144
# xrit_monitor_quality: a block record in float64
MONITOR_QUALITY_DTYPE = np.dtype([
    ("level", np.float64), ("dc", np.float64), ("flip_rate", np.float64), ("sat_rate", np.float64), ("neg_rate", np.float64),
    ("esn0_snv_db", np.float64), ("esn0_m2m4_db", np.float64), ("flags", np.uint32), ("reserved", np.uint32)])
assert MONITOR_QUALITY_DTYPE.itemsize == 64


class LinkMonitor(_Handle):
    """A stage behind the chain: per block of `block` symbols (a multiple of 64 in 64 .. 32768, 0 selects 16384) the sums
    from which `derive` gives the level, two Es/N0 estimates and the flip and saturation rates.  symbol_type SYMBOL_F32
    takes the chain's soft symbols, SYMBOL_I8 the quantiser's bytes.  The state lives in device memory: a stream may be
    cut into pushes anywhere.  There is no lock flag: an unlocked carrier and a weak link read alike."""
    _destroy = "xrit_monitor_destroy"

    def __init__(self, block=0, symbol_type=SYMBOL_F32, device=0):
        super().__init__()
        self.symbol_type = symbol_type
        _check(lib().xrit_monitor_create(C.byref(self._h), block, symbol_type, device))

    def rows(self, n):
        """The blocks a push of n symbols will complete; known on the host."""
        return lib().xrit_monitor_rows(self._h, n)

    def push(self, symbols):
        """-> the MONITOR_BLOCK_DTYPE records of the blocks these symbols complete."""
        a = np.ascontiguousarray(symbols, np.float32 if self.symbol_type == SYMBOL_F32 else np.int8).reshape(-1)
        rows = np.zeros(self.rows(len(a)), MONITOR_BLOCK_DTYPE)
        got = _sz()
        _check(lib().xrit_monitor_push(self._h, _p(a), len(a), _p(rows), len(rows), C.byref(got)))
        return rows[:got.value]

    def push_device(self, d_symbols_ptr, n, d_rows_ptr, cap_rows, d_summary_ptr=None, stream=None):
        """Device pointers; rows(n) records go to d_rows, 32 bytes of summary to d_summary when given.  Asynchronous on
        stream: it may be queued directly behind Demodulator.process_device or quantize_i8_device."""
        _check(lib().xrit_monitor_push_device(self._h, C.c_void_p(d_symbols_ptr), n, C.c_void_p(d_rows_ptr) if d_rows_ptr else None, cap_rows,
                                              C.c_void_p(d_summary_ptr) if d_summary_ptr else None, C.c_void_p(stream) if stream else None))

    def state(self):
        """Totals, the open record, the last sign and the histogram after the last call (a MONITOR_STATE_DTYPE scalar
        record); waits for that call."""
        out = np.zeros(1, MONITOR_STATE_DTYPE)
        _check(lib().xrit_monitor_get_state(self._h, _p(out)))
        return out[0]

    def reset(self):
        """The state zero: no open block, no last symbol."""
        _check(lib().xrit_monitor_reset(self._h))

    @staticmethod
    def derive(record, symbol_type=SYMBOL_F32):
        """One block record -> a MONITOR_QUALITY_DTYPE scalar record.  Plain host code: no device is asked for."""
        b = np.zeros(1, MONITOR_BLOCK_DTYPE)
        b[0] = record
        out = np.zeros(1, MONITOR_QUALITY_DTYPE)
        _check(lib().xrit_monitor_derive(_p(b), symbol_type, _p(out)))
        return out[0]
