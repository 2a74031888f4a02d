"""xritdemod_amd -- MI355X-native xRIT BPSK demodulation chain.

Python mirror of the C ABI in include/xritdemod_amd.h (ctypes).  The classes keep
the names and argument order of the SatHelper classes the reference builds at
/root/reference/demodulator/src/demodulator.cpp:443-450 and calls at
:138,:143,:148,:152,:156 (FirFilter, AGC, CostasLoop, ClockRecovery, Filters).

The compute path is the HIP library only: importing works without a GPU (so the
CPU test tier can check the ABI), but creating any stage or chain object raises
XritError when the library or a HIP device is missing.  There is no CPU fallback.
"""
from ._capi import (  # noqa: F401
    XritError, lib, lib_path, build, device_count, build_experiments, version,
    SAMPLE_FLOATIQ, SAMPLE_S16IQ, SAMPLE_S8IQ, SAMPLE_U8IQ,
    Filters, FirFilter, AGC, CostasLoop, ClockRecovery, RtlIngest, Demodulator, Group, LocalFabric, group_unique_id, DemodConfig, DemodStats,
    loop_sincosf, SynthParams as DeviceSynthParams, synth_generate_device, quantize_i8_device, sync_correlate, sync_correlate_device, sync_fix_frames, sync_fix_frames_device,
    LRIT_UW0, LRIT_UW2, HRIT_UW0, HRIT_UW2, FrameDecoder, FRAME_INFO_DTYPE, CADU_SIZE, BLOCK_SIZE, VCDU_SIZE,
    ChannelDemux, FRAME_STATS_DTYPE, DECODER_STATS_DTYPE, STATISTICS_WIRE_BYTES, N_VCID,
    PacketAssembler, PACKET_DTYPE, PACKETS_SUMMARY_DTYPE, PACKETS_STATS_DTYPE, packets_max_bytes,
    FileAssembler, FILE_PIECE_DTYPE, FILE_RECORD_DTYPE, FILES_SUMMARY_DTYPE, FILES_STATS_DTYPE, FILE_KEY_DTYPE,
    FrameSynchroniser, FRAMER_STATS_DTYPE, FRAMER_MAX_SYMBOLS,
    FrameLock, LOCK_STATS_DTYPE, LOCK_FULL, LOCK_SHORT, LOCK_MISS, LOCK_RECHECK, FLYWHEEL_RECHECK,
    FILE_BEGINS, FILE_ENDS, FILE_ABORTED, FILE_LENGTH_MATCH, RiceDecoder, rice_form, is_rice_coded, decode_file_lines,
    ImageDecoder, IMAGE_LINE_DTYPE, IMAGE_FILE_DTYPE, IMAGES_SUMMARY_DTYPE, IMAGES_STATS_DTYPE, IMAGE_KEY_DTYPE, images_max_bytes,
    ImageCanvas, CANVAS_FILE_DTYPE, CANVAS_SLOT_DTYPE, CANVAS_SEGMENT_DTYPE, CANVAS_KEY_DTYPE, CANVAS_SUMMARY_DTYPE, CANVAS_STATS_DTYPE,
    CANVAS_REASONS,
    ImageProduct, PRODUCT_IMAGE_DTYPE, PRODUCT_PARAMS_DTYPE, PRODUCT_SUMMARY_DTYPE, PRODUCT_TONES, PRODUCT_MAX_FACTOR,
    TONE_LINEAR, TONE_TABLE, TONE_EQUALISE, TONE_STRETCH,
    ImageProjector, GEO_NAV_DTYPE, GEO_GRID_DTYPE, GEO_POINT_DTYPE, GEO_SUMMARY_DTYPE, GEO_KINDS, GEO_MODES, GEO_MAX_DIM, GEO_OFF,
    GEO_EQUIRECT, GEO_MERCATOR, GEO_NEAREST, GEO_BILINEAR, geo_nav, geo_grid_tables, geo_parse_navigation, geo_pixel_to_lonlat,
    MapOverlay, OVERLAY_STYLE_DTYPE, OVERLAY_DRAW_SUMMARY_DTYPE, OVERLAY_BLEND_SUMMARY_DTYPE, OVERLAY_BREAK, OVERLAY_LIMIT, OVERLAY_MAX_DIM,
    OVERLAY_MAX_WIDTH, OVERLAY_LAYERS, OVERLAY_MAX_VERTICES, overlay_styles, overlay_quads, overlay_grid_points, overlay_densify,
    overlay_graticule,
    JpegEncoder, JPEG_RESULT_DTYPE, JPEG_MAX_BLOCKS, jpeg_bound, jpeg_quality_tables, jpeg_header,
    JpegDecoder, JPEGDEC_RECORD_DTYPE, JPEGDEC_SUMMARY_DTYPE, JPEGDEC_INFO_DTYPE, JPEGDEC_ITEM_DTYPE, JPEGDEC_MAX_BLOCKS, jpegdec_header,
    CarrierAcquirer, ACQUIRE_PARAMS_DTYPE, ACQUIRE_RECORD_DTYPE, ACQUIRE_STATE_DTYPE, ACQUIRE_OK, ACQUIRE_TOO_SHORT, ACQUIRE_WEAK,
    LinkMonitor, MONITOR_BLOCK_DTYPE, MONITOR_SUMMARY_DTYPE, MONITOR_STATE_DTYPE, MONITOR_QUALITY_DTYPE, SYMBOL_F32, SYMBOL_I8,
    MONITOR_NO_SIGNAL, MONITOR_NO_NOISE,
)
