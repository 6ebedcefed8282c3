"""
ctypes binding of libmrc_hip.so (include/mrc_hip.h).  Thin: argument marshalling and error mapping
only.  There is no fallback of any kind: if the shared library is missing the import fails, and if no
gfx950 device is usable `Handle()` raises -- nothing in this package computes on the CPU.
"""
import ctypes as C
import os
from types import SimpleNamespace

import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get("MRC_HIP_LIBRARY") or os.path.join(_HERE, "libmrc_hip.so")   # override: profiling builds

MRC_MAX_BANDS = 32
MRC_MAX_RATES = 16
MRC_MAX_CEILINGS = 256
MRC_MAX_PROBES = 9
MRC_ERR_INVALID = -1
MRC_ERR_NOMEM = -4
MRC_WINDOW_PCM16, MRC_WINDOW_F32, MRC_WINDOW_F64 = 0, 1, 2      # mrc_pac_store_decode_window's formats
MRC_MIX_MID, MRC_MIX_LEFT, MRC_MIX_RIGHT = 0, 1, 2               # mrc_pac_store_decode_window_mix's channels
MRC_MIX_EACH = 3                                                 # mrc_pac_store_block_energy: every channel of the file
MRC_FILTER_NORM_NONE, MRC_FILTER_NORM_SLANEY = 0, 1              # mrc_filterbank_line_weights' norms
MRC_OPT_STORE_SLAB_SAMPLES = 7
MRC_OPT_STORE_ROUTE_GROUP = 8                                    # reverb_route_fold_kernel: output channels per workgroup (0: per slab | 1 | 2)
MRC_MAX_STORE_ROUTE_CHANNELS = 16                                # mrc_pac_store_decode_window_routed: output channels of a row
MRC_ROUTE_NONE = -2                                              # ... a route that does not exist
MRC_STORE_REVERB_BLOCK = 1024                                    # mrc_pac_store_decode_window_reverb: the overlap-save hop B (N = 2 B)
MRC_MAX_STORE_IR_TAPS = 1 << 17                                  # mrc_pac_store_set_irs: taps of one impulse response
MRC_STFT_COMPLEX, MRC_STFT_POWER, MRC_STFT_BANK = 0, 1, 2        # mrc_pac_store_stft_window's modes
MRC_MAX_STFT_POINTS = 2048                                       # ... and its largest n_fft
# mrc_dev_helper_probe: name -> (MRC_PROBE_ id, words per element of in0 / in1 / in2, words per element of out)
PROBES = {
    "MOVES_I32": (1, (1, 1, 0), 8), "MOVES_U32": (2, (1, 1, 0), 8), "MOVES_F64": (3, (1, 1, 0), 8),
    "SUM_F64": (4, (1, 0, 0), 2), "MAX_F64": (5, (1, 0, 0), 1), "ROW_MAX": (6, (1, 0, 0), 1),
    "REDUCE_I32": (7, (1, 0, 0), 4), "FOLD4_F64": (8, (4, 0, 0), 1), "FOLD4_U32": (9, (4, 0, 0), 1),
    "FOLD2": (10, (2, 2, 0), 2), "SUM_BLOCK8": (11, (8, 0, 0), 8), "SUM_ALL9": (12, (9, 0, 0), 9),
    "SUM_ALL16": (13, (16, 0, 0), 16), "SUM_ALL17": (14, (17, 0, 0), 17), "SCAN_I32": (15, (1, 0, 0), 1),
    "SCAN_F64": (16, (1, 0, 0), 1), "ORDER_KEY": (17, (1, 0, 0), 2), "XCD": (18, (1, 1, 0), 1), "RCP": (19, (1, 0, 0), 2),
    "LINE_RATIO": (20, (1, 1, 0), 1), "EXP2_POLY": (21, (1, 0, 0), 1), "EXP2_TAB": (22, (1, 1, 0), 4),
    "TABLES": (23, (0, 0, 0), 4), "EXP2_DD": (24, (1, 1, 0), 1), "DD_ADD": (25, (2, 2, 0), 2), "ATAN_POS": (26, (1, 0, 0), 1),
    "SPL": (27, (1, 1, 0), 5), "MAG_CODE": (28, (1, 1, 0), 2), "SCALE_MANT": (29, (1, 1, 0), 4),
}
# array arguments travel as plain addresses (c_void_p prototypes): numpy's typed `data_as` costs ~2.3 us per array, which
# at thirteen arrays per call was a third of a one-block call through the drop-in seam; the names say what the C side expects
_i32p = _i64p = _f64p = _u8p = C.c_void_p


class MrcConfig(C.Structure):
    _fields_ = [("sample_rate", C.c_int32), ("n_mdct_lines", C.c_int32), ("n_short", C.c_int32),
                ("n_scale_bits", C.c_int32), ("n_mant_size_bits", C.c_int32), ("blksw_bits_a", C.c_int32),
                ("blksw_bits_b", C.c_int32), ("device_id", C.c_int32), ("target_bits_per_sample", C.c_double)]


class MrcError(RuntimeError):
    """code: the mrc_status the library returned (None for errors raised by the binding itself)"""
    code = None


def _preload_hip_runtime():
    """One HIP runtime per process.  PyTorch-ROCm wheels bundle their own libamdhip64.so (SONAME
    libamdhip64.so.7); if libmrc_hip.so pulled in /opt/rocm's copy first, a later `import torch` would
    load a second runtime that cannot see the GPU, and device pointers / streams could not be shared.
    So when torch is installed, its copy is loaded first (by path, nothing of torch is imported) and
    satisfies libmrc_hip.so's NEEDED entry; otherwise the system runtime is used."""
    import importlib.util
    try:
        spec = importlib.util.find_spec("torch")
    except (ImportError, ValueError):
        spec = None
    if spec is not None and spec.origin:
        cand = os.path.join(os.path.dirname(spec.origin), "lib", "libamdhip64.so")
        if os.path.exists(cand):
            C.CDLL(cand, mode=C.RTLD_GLOBAL)


def _load():
    if not os.path.exists(LIB_PATH):
        raise ImportError(
            "mrcaudiocodec_amd: %s is missing -- build it with `python -c 'import __graft_entry__ as g; g.build()'` "
            "or `make -C mrcaudiocodec_amd/csrc` (hipcc, gfx950).  There is no CPU fallback." % LIB_PATH)
    _preload_hip_runtime()
    lib = C.CDLL(LIB_PATH)
    H = C.c_void_p
    sig = {
        "mrc_version": (C.c_int, []),
        "mrc_device_count": (C.c_int, []),
        "mrc_default_config": (None, [C.POINTER(MrcConfig)]),
        "mrc_create": (C.c_int, [C.POINTER(MrcConfig), C.POINTER(H)]),
        "mrc_destroy": (None, [H]),
        "mrc_last_error": (C.c_char_p, [H]),
        "mrc_shape_bands": (C.c_int, [H, C.c_int, C.c_int, _i32p, _i32p]),
        "mrc_shape_budget": (C.c_int, [H, C.c_int, C.c_int, C.c_int, C.c_int32, _f64p]),
        "mrc_encode_mono": (C.c_int, [H, C.c_int64, C.c_int, C.c_int, _f64p, _i32p, _i32p, _i32p, _i32p, _i32p,
                                      _i32p, _f64p]),
        "mrc_encode_joint": (C.c_int, [H, C.c_int64, C.c_int, C.c_int, _f64p, _f64p, _i32p, _i32p, _i32p, _i32p,
                                       _i32p, _i32p, _i32p, _f64p]),
        "mrc_window": (C.c_int, [H, C.c_int64, C.c_int, C.c_int, _f64p, _f64p]),
        "mrc_mdct": (C.c_int, [H, C.c_int64, C.c_int, C.c_int, _f64p, C.c_int, _f64p, _i32p]),
        "mrc_smr": (C.c_int, [H, C.c_int64, C.c_int, C.c_int, _f64p, _f64p, _i32p, _f64p, _f64p]),
        "mrc_bitalloc": (C.c_int, [H, C.c_int64, C.c_int, C.c_int, _i32p, _f64p, _f64p, _i32p, _i32p]),
        "mrc_bitalloc_inplace": (C.c_int, [H, C.c_int64, C.c_int, C.c_int, _i32p, _f64p, _f64p, _i32p, _i32p]),
        "mrc_scale_factor": (C.c_int, [H, C.c_int64, C.c_int, _f64p, _i32p, _i32p]),
        "mrc_mantissa": (C.c_int, [H, C.c_int64, C.c_int, _f64p, _i32p, _i32p, _i32p]),
        "mrc_transient_peaks": (C.c_int, [H, C.c_int64, C.c_int, C.c_int, _f64p, _f64p, _f64p]),
        "mrc_transient_peaks_ex": (C.c_int, [H, C.c_int64, C.c_int, C.c_int, _f64p, C.c_void_p, C.c_int, _f64p]),
        "mrc_dev_transient_peaks": (C.c_int, [H, C.c_int64, C.c_int, C.c_int, _f64p, C.c_void_p, C.c_int, C.c_int64, C.c_void_p,
                                              C.c_void_p]),
        "mrc_stereo_masking_factor": (C.c_int, [H, C.c_int64, _f64p, _f64p, _f64p, _f64p, _f64p]),
        "mrc_ms_switch": (C.c_int, [H, C.c_int64, C.c_int, _i32p, _f64p, _f64p, _i32p]),
        "mrc_dev_mdct": (C.c_int, [H, C.c_int, C.c_int, C.c_int64, C.c_void_p, C.c_void_p, C.c_int64, C.c_void_p,
                                   C.c_void_p, C.c_void_p, C.c_void_p]),
        "mrc_dev_smr": (C.c_int, [H, C.c_int, C.c_int, C.c_int64, C.c_void_p, C.c_void_p, C.c_int64, C.c_void_p,
                                  C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]),
        "mrc_dev_masking": (C.c_int, [H, C.c_int, C.c_int, C.c_int64, C.c_void_p, C.c_void_p, C.c_int, C.c_int64] +
                            [C.c_void_p] * 7),
        "mrc_dev_helper_probe": (C.c_int, [H, C.c_int] + [C.c_void_p] * 4 + [C.c_int64, C.c_int64, C.c_int, C.c_void_p]),
        "mrc_dev_alloc_quant": (C.c_int, [H, C.c_int, C.c_int, C.c_int64, C.c_int] + [C.c_void_p] * 10),
        "mrc_dev_alloc_quant_chained": (C.c_int, [H, C.c_int, C.c_int, C.c_int64, C.c_int, C.c_int64, C.c_int] +
                                        [C.c_void_p] * 12),
        "mrc_vbr_record_width": (C.c_int, [C.c_int]),
        "mrc_dev_vbr_alloc": (C.c_int, [H, C.c_int, C.c_int, C.c_int64, C.c_int, C.c_double] + [C.c_void_p] * 11),
        "mrc_dev_vbr_profile": (C.c_int, [H, C.c_int, C.c_int, C.c_int64, C.c_int] + [C.c_void_p] * 8),
        "mrc_dev_vbr_pick": (C.c_int, [H, C.c_int, C.c_int, C.c_int64, C.c_int] + [C.c_void_p] * 12),
        "mrc_dev_encode": (C.c_int, [H, C.c_int, C.c_int, C.c_int64, C.c_void_p, C.c_void_p, C.c_int64] +
                           [C.c_void_p] * 10),
        "mrc_dev_encode_ex": (C.c_int, [H, C.c_int, C.c_int, C.c_int64, C.c_void_p, C.c_void_p, C.c_int, C.c_int64] +
                              [C.c_void_p] * 7 + [C.c_int] + [C.c_void_p] * 3),
        "mrc_encode_mono_blocks": (C.c_int, [H, C.c_int64, _f64p, _i32p, _i32p, _i32p, _i32p, _i32p, _i32p, _i32p, _i32p]),
        "mrc_encode_joint_blocks": (C.c_int, [H, C.c_int64, _f64p, _f64p, _i32p, _i32p, _i32p, _i32p, _i32p, _i32p, _i32p,
                                              _i32p, _i32p]),
        "mrc_encode_stream_pcm16": (C.c_int, [H, C.c_int64, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p,
                                              C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int64]),
        "mrc_encode_stream_pcm16_pac": (C.c_int, [H, C.c_int64, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_int64,
                                                  C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, _i64p, C.c_int64]),
        "mrc_host_alloc": (C.c_int, [C.POINTER(C.c_void_p), C.c_size_t]),
        "mrc_host_free": (C.c_int, [C.c_void_p]),
        "mrc_host_register": (C.c_int, [C.c_void_p, C.c_size_t]),
        "mrc_host_unregister": (C.c_int, [C.c_void_p]),
        "mrc_pcm_to_float": (C.c_int, [H, C.c_int64, C.c_void_p, _f64p]),
        "mrc_quantize_uniform": (C.c_int, [H, C.c_int64, C.c_int, _f64p, _i64p]),
        "mrc_bark": (C.c_int, [H, C.c_int64, _f64p, _f64p]),
        "mrc_get_kernel_ms": (C.c_int, [H, _f64p]),
        "mrc_huffman_gain": (C.c_int, [H, C.c_int64, C.c_int, C.c_int, C.c_int, _i32p, _i32p, _i32p, _i32p]),
        "mrc_dev_huffman_gain": (C.c_int, [H, C.c_int, C.c_int, C.c_int64, C.c_int] + [C.c_void_p] * 7),
        "mrc_dev_pack_blocks": (C.c_int, [H, C.c_int, C.c_int, C.c_int64, C.c_int, C.c_int, C.c_int] + [C.c_void_p] * 6 +
                                [C.c_int, C.c_void_p, C.c_int64, C.c_void_p, C.c_void_p, C.c_void_p, _i64p, C.c_void_p]),
        "mrc_dev_pack_status": (C.c_int, [H, _i64p, C.c_void_p]),
        "mrc_chain_out_bound": (C.c_int64, [H, C.c_int64, _i64p, _i32p, _i32p, C.c_int, C.c_int]),
        "mrc_chain_out_bound_ex": (C.c_int64, [H, C.c_int, C.c_int64, _i64p, _i32p, _i32p, C.c_int, C.c_int]),
        "mrc_encode_chained_stream_pcm16_pac": (C.c_int, [H, C.c_int64, C.c_void_p, C.c_void_p, C.c_int64, _i64p, _i64p, _i32p,
                                                          _i32p, _i32p, C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_int64,
                                                          _i64p, _i64p, _i32p, _i32p, _i64p]),
        "mrc_encode_chained_stream_pac": (C.c_int, [H, C.c_int64, C.c_void_p, C.c_void_p, C.c_int, C.c_int64, _i64p, _i64p,
                                                    _i32p, _i32p, _i32p, C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_int64,
                                                    _i64p, _i64p, _i32p, _i32p, _i64p]),
        "mrc_dev_encode_chained_pac": (C.c_int, [H, C.c_int64, C.c_void_p, C.c_void_p, C.c_int, C.c_int64, _i64p, _i64p,
                                                 _i32p, _i32p, _i32p, C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_int64,
                                                 _i64p, _i64p, _i32p, _i32p, _i64p, C.c_void_p]),
        "mrc_get_chain_ms": (C.c_int, [H, _f64p]),
        "mrc_encode_chained_ladder_pac": (C.c_int, [H, C.c_int, _f64p, C.c_int64, C.c_void_p, C.c_void_p, C.c_int, C.c_int64,
                                                    _i64p, _i64p, _i32p, _i32p, _i32p, C.c_int, C.c_int, C.c_void_p, C.c_void_p,
                                                    _i64p, _i64p, _i64p, _i32p, _i32p, _i64p]),
        "mrc_dev_encode_chained_ladder_pac": (C.c_int, [H, C.c_int, _f64p, C.c_int64, C.c_void_p, C.c_void_p, C.c_int, C.c_int64,
                                                        _i64p, _i64p, _i32p, _i32p, _i32p, C.c_int, C.c_int, C.c_void_p,
                                                        C.c_void_p, _i64p, _i64p, _i64p, _i32p, _i32p, _i64p, C.c_void_p]),
        "mrc_encode_chained_target_nmr_pac": (C.c_int, [H, C.c_int, _f64p, C.c_double, C.c_int64, C.c_void_p, C.c_void_p, C.c_int64,
                                                        _i64p, _i64p, _i32p, _i32p, C.c_int, C.c_void_p, C.c_void_p, C.c_int64,
                                                        _i64p, _i32p, _i32p, _f64p, _f64p, _i64p, _i64p, _i64p]),
        "mrc_dev_encode_chained_target_nmr_pac": (C.c_int, [H, C.c_int, _f64p, C.c_double, C.c_int64, C.c_void_p, C.c_void_p,
                                                            C.c_int64, _i64p, _i64p, _i32p, _i32p, C.c_int, C.c_void_p, C.c_void_p,
                                                            C.c_int64, _i64p, _i32p, _i32p, _f64p, _f64p, _i64p, _i64p, _i64p,
                                                            C.c_void_p]),
        "mrc_get_target_ms": (C.c_int, [H, _f64p]),
        "mrc_encode_vbr_nmr_pac": (C.c_int, [H, C.c_double, C.c_int64, C.c_void_p, C.c_void_p, C.c_int64, _i64p, _i64p, _i32p,
                                             _i32p, C.c_int, C.c_void_p, C.c_void_p, C.c_int64, _i64p, _f64p, _i64p, _i64p,
                                             _f64p, _f64p, _i64p, _i64p, _i64p]),
        "mrc_dev_encode_vbr_nmr_pac": (C.c_int, [H, C.c_double, C.c_int64, C.c_void_p, C.c_void_p, C.c_int64, _i64p, _i64p,
                                                 _i32p, _i32p, C.c_int, C.c_void_p, C.c_void_p, C.c_int64, _i64p, _f64p, _i64p,
                                                 _i64p, _f64p, _f64p, _i64p, _i64p, _i64p, C.c_void_p]),
        "mrc_get_vbr_ms": (C.c_int, [H, _f64p]),
        "mrc_encode_vbr_size_pac": (C.c_int, [H, C.c_double, C.c_double, C.c_int, _i64p, C.c_int64, C.c_void_p, C.c_void_p,
                                              C.c_int64, _i64p, _i64p, _i32p, _i32p, C.c_int, C.c_void_p, C.c_void_p, C.c_int64,
                                              _i64p, _i32p, _f64p, _f64p, _i32p, _i32p, _i32p, _i64p, _i64p, _i64p, _f64p, _f64p,
                                              _i64p, _i64p, _i64p]),
        "mrc_dev_encode_vbr_size_pac": (C.c_int, [H, C.c_double, C.c_double, C.c_int, _i64p, C.c_int64, C.c_void_p, C.c_void_p,
                                                  C.c_int64, _i64p, _i64p, _i32p, _i32p, C.c_int, C.c_void_p, C.c_void_p,
                                                  C.c_int64, _i64p, _i32p, _f64p, _f64p, _i32p, _i32p, _i32p, _i64p, _i64p, _i64p,
                                                  _f64p, _f64p, _i64p, _i64p, _i64p, C.c_void_p]),
        "mrc_get_vbr_size_ms": (C.c_int, [H, _f64p]),
        "mrc_pac_read_header": (C.c_int, [_u8p, C.c_int64, C.POINTER(MrcConfig), _i32p, C.POINTER(C.c_uint32), _i64p]),
        "mrc_pac_scan_chunks": (C.c_int64, [_u8p, C.c_int64, C.c_int64, _i64p, C.c_int64]),
        "mrc_unpack_blocks": (C.c_int, [C.POINTER(MrcConfig), C.c_int64, C.c_int, C.c_int, _u8p, C.c_int64, _i64p] +
                              [_i32p] * 8),
        "mrc_decode": (C.c_int, [H, C.c_int64, C.c_int, C.c_int, C.c_int, _i32p, _i32p, _i32p, _i32p, _i32p, _f64p]),
        "mrc_dev_decode": (C.c_int, [H, C.c_int, C.c_int, C.c_int64, C.c_int] + [C.c_void_p] * 9),
        "mrc_pcm16": (C.c_int, [H, C.c_int64, _f64p, C.POINTER(C.c_int16)]),
        "mrc_dev_pcm16": (C.c_int, [H, C.c_int64, C.c_void_p, C.c_void_p, C.c_void_p]),
        "mrc_band_table": (C.c_int, [C.POINTER(MrcConfig), C.c_int, C.c_int, _i32p, _i32p]),
        "mrc_pack_bound": (C.c_int64, [C.POINTER(MrcConfig), C.c_int, C.c_int, C.c_int, C.c_int]),
        "mrc_pac_header": (C.c_int, [C.POINTER(MrcConfig), C.c_int, C.c_uint32, _u8p, C.c_int64, _i64p]),
        "mrc_pack_set_threads": (C.c_int, [C.c_int]),
        "mrc_pack_get_threads": (C.c_int, []),
        "mrc_pack_blocks_ex": (C.c_int, [C.POINTER(MrcConfig), C.c_int64, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, _i32p,
                                         _i32p, _i32p, _i32p, _i32p, C.c_void_p, C.c_int, _u8p, C.c_int64, _i64p, _i32p, _i32p]),
        "mrc_pack_blocks_with_tables": (C.c_int, [C.POINTER(MrcConfig), C.c_int64, C.c_int, C.c_int, C.c_int, _i32p, _i32p,
                                                  _i32p, _i32p, _i32p, _u8p, C.c_int64, _i64p]),
        "mrc_pack_joint_blocks_with_tables": (C.c_int, [C.POINTER(MrcConfig), C.c_int64, C.c_int, C.c_int, _i32p, _i32p,
                                                        _i32p, _i32p, _i32p, _i32p, _u8p, C.c_int64, _i64p]),
        "mrc_pack_blocks": (C.c_int, [C.POINTER(MrcConfig), C.c_int64, C.c_int, C.c_int, C.c_int, C.c_int, _i32p,
                                      _i32p, _i32p, _i32p, _u8p, C.c_int64, _i64p, _i32p, _i32p]),
        "mrc_pack_joint_blocks": (C.c_int, [C.POINTER(MrcConfig), C.c_int64, C.c_int, C.c_int, C.c_int, _i32p, _i32p,
                                            _i32p, _i32p, _i32p, _u8p, C.c_int64, _i64p, _i32p, _i32p]),
        "mrc_chain_fetch_output": (C.c_int, [H, C.c_void_p, C.c_int64, _i64p]),
        "mrc_get_sensitivity": (C.c_int, [H, _i64p, C.c_int]),
        "mrc_set_timing": (C.c_int, [H, C.c_int]),
        "mrc_set_option": (C.c_int, [H, C.c_int, C.c_int]),
        "mrc_get_option": (C.c_int, [H, C.c_int, _i32p]),
        "mrc_get_stage_ms": (C.c_int, [H, _f64p]),
        "mrc_dev_unpack_blocks": (C.c_int, [H, C.c_int64, C.c_int, C.c_int, C.c_void_p, C.c_int64] + [C.c_void_p] * 10),
        "mrc_decode_pac_pcm16": (C.c_int, [H, C.c_int64, _u8p, _i64p, C.c_void_p, C.c_int64, _i64p, _i32p]),
        "mrc_get_decode_ms": (C.c_int, [H, _f64p]),
        "mrc_pac_nmr": (C.c_int, [H, C.c_int64, _u8p, _i64p, C.c_void_p, _i64p, _i64p, _i64p, _f64p, _f64p, _i64p, _i64p,
                                  _i64p, C.c_int64, _i32p, _f64p, _f64p]),
        "mrc_get_nmr_ms": (C.c_int, [H, _f64p]),
        "mrc_pac_index": (C.c_int, [C.POINTER(MrcConfig), _u8p, C.c_int64, _i32p, _i64p, _i64p, C.c_int64, _i64p, _i32p, _i32p,
                                    _i64p]),
        "mrc_pac_store_create": (C.c_int, [H, C.c_int64, _u8p, _i64p, C.POINTER(C.c_void_p)]),
        "mrc_pac_store_destroy": (None, [C.c_void_p]),
        "mrc_pac_store_info": (C.c_int, [C.c_void_p, _i64p, _i32p, _i64p, _i64p, _i64p]),
        "mrc_pac_store_decode_window": (C.c_int, [C.c_void_p, C.c_int64, _i64p, _i64p, C.c_int64, C.c_int, C.c_int, C.c_void_p,
                                                  C.c_void_p]),
        "mrc_pac_store_decode_window_reduced": (C.c_int, [C.c_void_p, C.c_int, C.c_int64, _i64p, _i64p, C.c_int64, C.c_int,
                                                          C.c_int, C.c_void_p, C.c_void_p]),
        "mrc_pac_store_decode_window_mix": (C.c_int, [C.c_void_p, C.c_int, C.c_int, C.c_int64, _i64p, _i64p, C.c_int64, C.c_int,
                                                      C.c_void_p, C.c_void_p]),
        "mrc_pac_store_block_energy": (C.c_int, [C.c_void_p, C.c_int, C.c_int, C.c_int64, _i64p, _i64p, C.c_int64, _i64p, _f64p,
                                                 C.c_void_p]),
        "mrc_synthesis_shape": (C.c_int, [C.c_int, C.c_int, C.c_int]),
        "mrc_band_line_ranges": (C.c_int, [C.c_double, C.c_int, C.c_int, C.c_int, _f64p, _i32p]),
        "mrc_pac_store_band_energy_window": (C.c_int, [C.c_void_p, C.c_int, C.c_int64, _i64p, _i64p, C.c_int64, C.c_int64, C.c_int,
                                                       _f64p, C.c_int, C.c_int, C.c_void_p, C.c_void_p]),
        "mrc_filterbank_line_weights": (C.c_int, [C.c_double, C.c_int, C.c_int, C.c_int, _f64p, C.c_int, _i32p, _i32p, C.c_int64,
                                                  _f64p, _i64p]),
        "mrc_pac_store_filterbank_window": (C.c_int, [C.c_void_p, C.c_int, C.c_int64, _i64p, _i64p, C.c_int64, C.c_int64, C.c_int,
                                                      _f64p, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_void_p]),
        "mrc_resample_taps": (C.c_int, [C.c_int, C.c_int, C.c_int, C.c_double, _i32p, _f64p]),
        "mrc_pac_store_decode_window_resampled": (C.c_int, [C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_double,
                                                            C.c_int64, _i64p, _i64p, C.c_int64, C.c_int, C.c_int, C.c_void_p,
                                                            C.c_void_p]),
        "mrc_pac_store_decode_window_sum": (C.c_int, [C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_double, C.c_int64,
                                                      _i64p, _i64p, _i64p, _f64p, C.c_int64, C.c_int, C.c_int, C.c_void_p,
                                                      C.c_void_p]),
        "mrc_pac_store_decode_window_shaped": (C.c_int, [C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_double, C.c_int,
                                                         _f64p, _f64p, C.c_int64, _i64p, _i64p, _i64p, _f64p, C.c_int64, C.c_int,
                                                         C.c_int, C.c_void_p, C.c_void_p]),
        "mrc_pac_store_decode_window_speeds": (C.c_int, [C.c_void_p, C.c_int, C.c_int, C.c_int, _i32p, _i32p, C.c_int, C.c_double,
                                                         C.c_int, _f64p, _f64p, C.c_int64, _i64p, _i64p, _i64p, _f64p, _i32p,
                                                         C.c_int64, C.c_int, C.c_int, C.c_void_p, C.c_void_p]),
        "mrc_pac_store_stats": (C.c_int, [C.c_void_p, _i64p, _f64p]),
        "mrc_pac_store_set_irs": (C.c_int, [C.c_void_p, C.c_int64, _i64p, _f64p]),
        "mrc_pac_store_ir_info": (C.c_int, [C.c_void_p, _i64p, _i64p]),
        "mrc_pac_store_decode_window_reverb": (C.c_int, [C.c_void_p, C.c_int, C.c_int, C.c_int, _i32p, _i32p, C.c_int, C.c_double,
                                                         C.c_int, _f64p, _f64p, C.c_int64, _i64p, _i64p, _i64p, _f64p, _i32p, _i32p,
                                                         C.c_int64, C.c_int, C.c_int, C.c_void_p, C.c_void_p]),
        "mrc_pac_store_reverb_ms": (C.c_int, [C.c_void_p, _f64p]),
        "mrc_pac_store_stft_window": (C.c_int, [C.c_void_p, C.c_int, C.c_int, C.c_int, _i32p, _i32p, C.c_int, C.c_double,
                                                C.c_int, _f64p, _f64p, C.c_int64, _i64p, _i64p, _i64p, _f64p, _i32p, _i32p,
                                                C.c_int, _f64p, C.c_int64, C.c_int64, C.c_int, C.c_int, _f64p, C.c_int, C.c_int,
                                                C.c_void_p, C.c_void_p]),
        "mrc_pac_store_stft_ms": (C.c_int, [C.c_void_p, _f64p]),
        "mrc_pac_store_decode_window_routed": (C.c_int, [C.c_void_p, C.c_int, C.c_int, C.c_int, _i32p, _i32p, C.c_int, C.c_double,
                                                         C.c_int, _f64p, _f64p, C.c_int64, _i64p, _i64p, _i64p, _i32p, _f64p, _i32p,
                                                         C.c_int64, C.c_int, C.c_int, C.c_void_p, C.c_void_p]),
        "mrc_pac_store_stft_window_routed": (C.c_int, [C.c_void_p, C.c_int, C.c_int, C.c_int, _i32p, _i32p, C.c_int, C.c_double,
                                                       C.c_int, _f64p, _f64p, C.c_int64, _i64p, _i64p, _i64p, _i32p, _f64p, _i32p,
                                                       C.c_int, _f64p, C.c_int64, C.c_int64, C.c_int, C.c_int, _f64p, C.c_int, C.c_int,
                                                       C.c_void_p, C.c_void_p]),
        "mrc_pac_store_route_info": (C.c_int, [C.c_void_p, _i64p]),
        "mrc_pac_store_decode_window_spans": (C.c_int, [C.c_void_p, C.c_int, C.c_int, C.c_int, _i32p, _i32p, C.c_int, C.c_double,
                                                        C.c_int, _f64p, _f64p, C.c_int64, _i64p, _i64p, _i64p, _f64p, _i32p, _i32p,
                                                        _i64p, _i64p, _i64p, _i64p, C.c_int64, C.c_int, C.c_int, C.c_void_p,
                                                        C.c_void_p]),
        "mrc_pac_store_stft_window_spans": (C.c_int, [C.c_void_p, C.c_int, C.c_int, C.c_int, _i32p, _i32p, C.c_int, C.c_double,
                                                      C.c_int, _f64p, _f64p, C.c_int64, _i64p, _i64p, _i64p, _f64p, _i32p, _i32p,
                                                      _i64p, _i64p, _i64p, _i64p, C.c_int, _f64p, C.c_int64, C.c_int64, C.c_int,
                                                      C.c_int, _f64p, C.c_int, C.c_int, C.c_void_p, C.c_void_p]),
    }
    for name, (res, args) in sig.items():
        fn = getattr(lib, name)          # AttributeError here = the library does not export the header's symbol
        fn.restype = res
        fn.argtypes = args
    return lib, tuple(sig)


lib, EXPORTS = _load()


def _f64(a):
    return np.ascontiguousarray(a, dtype=np.float64)


def _i32(a):
    return np.ascontiguousarray(a, dtype=np.int32)


def _reservoir(reservoir_in, n):
    """reservoir_in as int32 [n] (None stays None); the C side reads n values from it."""
    if reservoir_in is None:
        return None
    r = _i32(np.asarray(reservoir_in).reshape(-1))
    if r.shape != (n,):
        raise ValueError("reservoir_in must hold one value per block (%d), got %d" % (n, r.size))
    return r


def _p(a, typ):
    return None if a is None else a.ctypes.data


def vp(arr):
    return None if arr is None else arr.ctypes.data_as(C.c_void_p)


def nmr_layout(bufs, sources):
    """The host side of mrc_pac_nmr's arguments: bufs (a list of bytes-like `.pac` files) -> one byte buffer and
    file_offset; sources (a list or tuple, one int16 [nCh][n] array per file; the same object may repeat and is then
    staged once) -> one planar int16 buffer with src_offset / src_stride / src_frames per file.  Each source must have
    exactly the channel count its file's header names: the library reads nCh rows of src_frames samples from the
    address it is given and cannot see where the caller's array ends.  Also returns the number of chunks of all files
    (the entry count of the call).  Raises ValueError before anything is read past an array."""
    if not isinstance(sources, (list, tuple)):
        raise ValueError("pac_nmr: sources must be a list with one int16 [nCh][n] array per file")
    n = len(bufs)
    if len(sources) != n:
        raise ValueError("pac_nmr: one source per file (%d files, %d sources)" % (n, len(sources)))
    sizes = np.fromiter((len(b) for b in bufs), dtype=np.int64, count=n)
    file_offset = np.zeros(n + 1, np.int64)
    np.cumsum(sizes, out=file_offset[1:])
    data = np.frombuffer(b"".join(bytes(b) for b in bufs), np.uint8) if n else np.zeros(1, np.uint8)
    n_entries = 0
    planes, where = [], {}
    src_offset = np.zeros(max(n, 1), np.int64)
    src_stride = np.zeros(max(n, 1), np.int64)
    src_frames = np.zeros(max(n, 1), np.int64)
    total = 0
    cfg, nch, ns, doff = MrcConfig(), C.c_int32(), C.c_uint32(), C.c_int64()
    for f, s in enumerate(sources):
        if id(s) not in where:
            a = np.ascontiguousarray(np.asarray(s))
            if a.ndim == 1:
                a = a[None]
            if a.dtype != np.int16 or a.ndim != 2:
                raise ValueError("pac_nmr: source %d is not an int16 [nCh][n] array" % f)
            where[id(s)] = (total, a.shape[1], a.shape[0])
            planes.append(a.reshape(-1))
            total += a.size
        src_offset[f], src_frames[f], rows = where[id(s)]
        src_stride[f] = src_frames[f]
        raw = data[file_offset[f]:file_offset[f + 1]]
        # (a file whose header or chunks do not read is refused by the library before it touches any source)
        if raw.size and lib.mrc_pac_read_header(raw.ctypes.data, raw.size, C.byref(cfg), C.byref(nch), C.byref(ns),
                                                C.byref(doff)) == 0:
            if rows != nch.value:
                raise ValueError("pac_nmr: file %d has %d channel(s), its source %d row(s)" % (f, nch.value, rows))
            n_entries += max(0, int(lib.mrc_pac_scan_chunks(raw.ctypes.data, raw.size, doff.value, None, 0)))
    # (one distinct source -- one file, or the rungs of a ladder -- is passed as it is, without a copy)
    src = planes[0] if len(planes) == 1 else np.concatenate(planes) if planes else np.zeros(1, np.int16)
    return data, file_offset, src, src_offset, src_stride, src_frames, n_entries


class ChainSchedule:
    """The block schedule of a chained encode as the C ABI takes it (block_start [nStreams + 1], offset / a / b per block),
    built ONCE from per-stream shape lists or arrays and reused from call to call."""

    def __init__(self, shapes):
        self.start, self.offset, self.a, self.b = Handle._chain_schedule(shapes)

    def __len__(self):
        return len(self.start) - 1


class Handle:
    """One mrc_handle: a device, a stream, the constant tables of the block shapes."""

    def __init__(self, sample_rate=48000, n_mdct_lines=1024, n_short=128, n_scale_bits=4, n_mant_size_bits=4,
                 target_bits_per_sample=2.86, blksw_bits_a=1, blksw_bits_b=1, device_id=0):
        cfg = MrcConfig()
        lib.mrc_default_config(C.byref(cfg))
        cfg.sample_rate = int(sample_rate)
        cfg.n_mdct_lines = int(n_mdct_lines)
        cfg.n_short = int(n_short)
        cfg.n_scale_bits = int(n_scale_bits)
        cfg.n_mant_size_bits = int(n_mant_size_bits)
        cfg.target_bits_per_sample = float(target_bits_per_sample)
        cfg.blksw_bits_a = int(blksw_bits_a)
        cfg.blksw_bits_b = int(blksw_bits_b)
        cfg.device_id = int(device_id)
        self.cfg = cfg
        self._h = C.c_void_p()
        rc = lib.mrc_create(C.byref(cfg), C.byref(self._h))
        if rc != 0:
            msg = lib.mrc_last_error(None)
            self._h = None
            raise MrcError("mrc_create failed (%d): %s" % (rc, msg.decode() if msg else "?"))
        self._bands = {}

    def close(self):
        if getattr(self, "_h", None):
            lib.mrc_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def _check(self, rc):
        if rc != 0:
            msg = lib.mrc_last_error(self._h)
            err = MrcError("libmrc_hip error %d: %s" % (rc, msg.decode() if msg else "?"))
            err.code = rc
            raise err

    # ---- shape queries
    def bands(self, a, b):
        """nLines per scale-factor band of shape (a,b) (int32 array)."""
        key = (int(a), int(b))
        if key not in self._bands:
            n = C.c_int32()
            buf = np.zeros(MRC_MAX_BANDS, dtype=np.int32)
            self._check(lib.mrc_shape_bands(self._h, key[0], key[1], C.byref(n), _p(buf, _i32p)))
            self._bands[key] = buf[:n.value].copy()
        return self._bands[key]

    def budget(self, a, b, joint, reservoir=0):
        v = C.c_double()
        self._check(lib.mrc_shape_budget(self._h, int(a), int(b), int(bool(joint)), int(reservoir), C.byref(v)))
        return v.value

    # ---- host entry points
    def encode_mono(self, blocks, a, b, reservoir_in=None, want_mdct=False):
        blocks = _f64(blocks)
        n, N = blocks.shape
        if N != a + b:
            raise ValueError("blocks must be [n][a+b]")
        nb, half = len(self.bands(a, b)), N // 2
        res_in = _reservoir(reservoir_in, n)
        out = dict(overall_scale=np.empty(n, np.int32), scale_factor=np.empty((n, nb), np.int32),
                   bit_alloc=np.empty((n, nb), np.int32), mantissa=np.empty((n, half), np.int32),
                   reservoir_out=np.empty(n, np.int32))
        mdct = np.empty((n, half), np.float64) if want_mdct else None
        self._check(lib.mrc_encode_mono(self._h, n, a, b, _p(blocks, _f64p), _p(res_in, _i32p),
                                        _p(out["overall_scale"], _i32p), _p(out["scale_factor"], _i32p),
                                        _p(out["bit_alloc"], _i32p), _p(out["mantissa"], _i32p),
                                        _p(out["reservoir_out"], _i32p), _p(mdct, _f64p)))
        if want_mdct:
            out["mdct"] = mdct
        return out

    def encode_joint(self, left, right, a, b, reservoir_in=None, want_mdct=False):
        left, right = _f64(left), _f64(right)
        n, N = left.shape
        if N != a + b or right.shape != left.shape:
            raise ValueError("left/right must be [n][a+b]")
        nb, half = len(self.bands(a, b)), N // 2
        res_in = _reservoir(reservoir_in, n)
        out = dict(overall_scale=np.empty((n, 4), np.int32), ms_switch=np.empty((n, nb), np.int32),
                   scale_factor=np.empty((n, 2, nb), np.int32), bit_alloc=np.empty((n, 2, nb), np.int32),
                   mantissa=np.empty((n, 2, half), np.int32), reservoir_out=np.empty(n, np.int32))
        mdct = np.empty((n, 4, half), np.float64) if want_mdct else None
        self._check(lib.mrc_encode_joint(self._h, n, a, b, _p(left, _f64p), _p(right, _f64p), _p(res_in, _i32p),
                                         _p(out["overall_scale"], _i32p), _p(out["ms_switch"], _i32p),
                                         _p(out["scale_factor"], _i32p), _p(out["bit_alloc"], _i32p),
                                         _p(out["mantissa"], _i32p), _p(out["reservoir_out"], _i32p),
                                         _p(mdct, _f64p)))
        if want_mdct:
            out["mdct"] = mdct
        return out

    def encode_blocks(self, left, a, b, right=None, reservoir_in=None):
        """Blocks of MIXED shapes in one call (mrc_encode_mono_blocks / mrc_encode_joint_blocks): `left` (and `right`)
        is a list of 1-D arrays, block i holding a[i] + b[i] samples.  Outputs have fixed strides: scale_factor /
        bit_alloc [n][streams][MRC_MAX_BANDS], ms_switch [n][MRC_MAX_BANDS], mantissa [n][streams][n_mdct_lines]."""
        a, b = _i32(a), _i32(b)
        n = len(a)
        if len(b) != n or len(left) != n or (right is not None and len(right) != n):
            raise ValueError("one (a, b) pair and one block per entry expected")
        for i in range(n):
            if len(left[i]) != a[i] + b[i] or (right is not None and len(right[i]) != a[i] + b[i]):
                raise ValueError("block %d does not hold a + b = %d samples" % (i, a[i] + b[i]))
        packed_l = _f64(np.concatenate([np.asarray(x, dtype=np.float64) for x in left])) if n else np.zeros(0)
        res_in = _reservoir(reservoir_in, n)
        L = self.cfg.n_mdct_lines
        ns, nsig = (2, 4) if right is not None else (1, 1)
        out = dict(overall_scale=np.empty((n, nsig) if right is not None else n, np.int32),
                   scale_factor=np.empty((n, ns, MRC_MAX_BANDS), np.int32), bit_alloc=np.empty((n, ns, MRC_MAX_BANDS), np.int32),
                   mantissa=np.empty((n, ns, L), np.int32), reservoir_out=np.empty(n, np.int32))
        if right is None:
            self._check(lib.mrc_encode_mono_blocks(self._h, n, _p(packed_l, _f64p), _p(a, _i32p), _p(b, _i32p),
                                                   _p(res_in, _i32p), _p(out["overall_scale"], _i32p),
                                                   _p(out["scale_factor"], _i32p), _p(out["bit_alloc"], _i32p),
                                                   _p(out["mantissa"], _i32p), _p(out["reservoir_out"], _i32p)))
        else:
            packed_r = _f64(np.concatenate([np.asarray(x, dtype=np.float64) for x in right])) if n else np.zeros(0)
            out["ms_switch"] = np.empty((n, MRC_MAX_BANDS), np.int32)
            self._check(lib.mrc_encode_joint_blocks(self._h, n, _p(packed_l, _f64p), _p(packed_r, _f64p), _p(a, _i32p),
                                                    _p(b, _i32p), _p(res_in, _i32p), _p(out["overall_scale"], _i32p),
                                                    _p(out["ms_switch"], _i32p), _p(out["scale_factor"], _i32p),
                                                    _p(out["bit_alloc"], _i32p), _p(out["mantissa"], _i32p),
                                                    _p(out["reservoir_out"], _i32p)))
        return out

    def _stream_pcm16(self, pcm_left, pcm_right):
        """int16 stream(s) [(n + 1) * L] of the encode_stream_pcm16* calls -> (left, right or None, n)"""
        L = self.cfg.n_mdct_lines
        pl = np.ascontiguousarray(pcm_left, dtype=np.int16)
        n = pl.size // L - 1
        if pl.ndim != 1 or pl.size != (n + 1) * L or n < 0:
            raise ValueError("pcm_left must be int16 [(n_frames + 1) * %d]" % L)
        pr = None
        if pcm_right is not None:
            pr = np.ascontiguousarray(pcm_right, dtype=np.int16)
            if pr.shape != pl.shape:
                raise ValueError("pcm_right must match pcm_left")
        return pl, pr, n

    def encode_stream_pcm16(self, pcm_left, pcm_right=None, reservoir_in=None, chunk_frames=0, out=None):
        """mrc_encode_stream_pcm16: int16 PCM stream(s) [(n+1) * L] in host memory -> codes in host memory, long
        blocks, pipelined over three HIP streams.  `out` may hold preallocated (ideally page-locked, see
        pinned_empty) arrays to write into; the mantissa plane is uint16."""
        L = self.cfg.n_mdct_lines
        pl, pr, n = self._stream_pcm16(pcm_left, pcm_right)
        joint = pr is not None
        nb = len(self.bands(L, L))
        ns, nsig = (2, 4) if joint else (1, 1)
        want = dict(overall_scale=((n, nsig), np.int32), scale_factor=((n, ns, nb), np.int32),
                    bit_alloc=((n, ns, nb), np.int32), mantissa=((n, ns, L), np.uint16), reservoir_out=((n,), np.int32))
        if joint:
            want["ms_switch"] = ((n, nb), np.int32)
        res = {}
        for k, (shape, dt) in want.items():
            arr = None if out is None else out.get(k)
            if arr is None:
                arr = np.empty(shape, dt)
            elif arr.shape != shape or arr.dtype != dt or not arr.flags.c_contiguous:
                raise ValueError("out[%r] must be a C-contiguous %s array of shape %s" % (k, np.dtype(dt).name, shape))
            res[k] = arr
        res_in = _reservoir(reservoir_in, n)
        self._check(lib.mrc_encode_stream_pcm16(self._h, n, vp(pl), vp(pr), vp(res_in), vp(res["overall_scale"]),
                                                vp(res.get("ms_switch")), vp(res["scale_factor"]), vp(res["bit_alloc"]),
                                                vp(res["mantissa"]), vp(res["reservoir_out"]), int(chunk_frames)))
        return res

    def encode_stream_pcm16_pac(self, pcm_left, pcm_right=None, reservoir_in=None, use_huffman=True, chunk_frames=0,
                                out=None, bytes_per_chunk=None):
        """mrc_encode_stream_pcm16_pac: int16 PCM stream(s) [(n+1) * L] in host memory -> the `.pac` chunk bytes of the n
        long blocks in host memory (encode kernels + Huffman pricing + bit packing on the device, pipelined).  `out` may hold
        a preallocated (ideally page-locked) uint8 array `bytes`; too small a buffer is retried once at the worst-case size.
        -> dict: bytes (the used prefix), block_offset [n + 1], huff_table / bits_saved [n][channels], reservoir_out [n]."""
        L = self.cfg.n_mdct_lines
        pl, pr, n = self._stream_pcm16(pcm_left, pcm_right)
        joint = pr is not None
        nch = 2 if joint else 1
        bound = int(lib.mrc_pack_bound(C.byref(self.cfg), L, L, 1, 1 if joint else 0))
        buf = None if out is None else out.get("bytes")
        if buf is not None and (buf.dtype != np.uint8 or buf.ndim != 1 or not buf.flags.c_contiguous):
            raise ValueError("out['bytes'] must be a C-contiguous 1-D uint8 array")
        if buf is None:
            buf = np.empty(max(1, n * nch * int(bytes_per_chunk or L) + 4096), np.uint8)
        offs = np.zeros(n + 1, np.int64)
        table, saved = np.zeros((n, nch), np.int32), np.zeros((n, nch), np.int32)
        res_out = np.zeros(n, np.int32)
        res_in = _reservoir(reservoir_in, n)
        total = np.zeros(1, np.int64)
        for attempt in (0, 1):
            rc = lib.mrc_encode_stream_pcm16_pac(self._h, n, vp(pl), vp(pr), vp(res_in), 1 if use_huffman else 0, vp(buf),
                                                 buf.size, vp(offs), vp(table), vp(saved), vp(res_out),
                                                 total.ctypes.data_as(_i64p), int(chunk_frames))
            if rc == MRC_ERR_NOMEM and attempt == 0 and buf.size < n * nch * bound:
                buf = np.empty(n * nch * bound, np.uint8)
                continue
            self._check(rc)
            break
        return {"bytes": buf[:int(total[0])], "block_offset": offs, "huff_table": table, "bits_saved": saved,
                "reservoir_out": res_out}

    # ---- chained stream encode (the reference's whole encode loop in one call)
    @staticmethod
    def _chain_schedule(shapes):
        """shapes[s] = [(offset, a, b), ...] (or an int array [n][3]) -> block_start, offset, a, b arrays."""
        if isinstance(shapes, ChainSchedule):
            return shapes.start, shapes.offset, shapes.a, shapes.b
        counts = [len(sh) for sh in shapes]
        start = np.zeros(len(shapes) + 1, np.int64)
        start[1:] = np.cumsum(counts)
        flat = np.concatenate([np.asarray(sh, dtype=np.int64).reshape(-1, 3) for sh in shapes]) if counts and sum(counts) \
            else np.zeros((0, 3), np.int64)
        return (start, np.ascontiguousarray(flat[:, 0]), np.ascontiguousarray(flat[:, 1], dtype=np.int32),
                np.ascontiguousarray(flat[:, 2], dtype=np.int32))

    def _chain_args(self, pcm_left, pcm_right, shapes, use_huffman, with_flush, num_samples, device):
        """What encode_chained_pac and encode_chained_pac_ladder share.  -> namespace: n_streams, nch, n_blocks, n_items;
        pcm = the arguments (left, right, sample_format, stride), from the host arrays [nStreams][stride] or from `device`;
        head / opts = the schedule arguments in front of and behind reservoir_in; bound() = the worst-case bytes of one rate."""
        start, off, a, b = self._chain_schedule(shapes)
        n_streams = len(start) - 1
        keep = None
        if device is None:
            mono = pcm_right is None
            pl = np.atleast_2d(pcm_left)
            dt = np.int16 if pl.dtype == np.int16 else np.float64
            pl = np.ascontiguousarray(pl, dtype=dt)
            pr = None if mono else np.ascontiguousarray(np.atleast_2d(pcm_right), dtype=dt)
            if (not mono and pl.shape != pr.shape) or pl.ndim != 2 or pl.shape[0] != n_streams:
                raise ValueError("pcm_left / pcm_right must be [nStreams][stride], one row per shape list")
            keep, pcm = (pl, pr), (vp(pl), vp(pr), 1 if dt == np.int16 else 0, pl.shape[1])
        else:
            mono, pcm = device[1] is None, (device[0], device[1], int(device[2]), int(device[3]))
        nch = 1 if mono else 2
        ns = None if num_samples is None else np.ascontiguousarray(num_samples, dtype=np.uint32)
        if ns is not None and ns.shape != (n_streams,):
            raise ValueError("num_samples: one value per stream")

        def bound():
            v = self.chain_out_bound(start, a, b, with_flush, ns is not None, nch)
            if v < 0:
                raise MrcError("mrc_chain_out_bound failed (%d): block shape out of range" % v)
            return v
        return SimpleNamespace(n_streams=n_streams, nch=nch, n_blocks=int(off.size), pcm=pcm, bound=bound,
                               n_items=len(off) + (nch * n_streams if with_flush else 0),
                               head=(_p(start, _i64p), _p(off, _i64p), _p(a, _i32p), _p(b, _i32p)),
                               opts=(1 if use_huffman else 0, 1 if with_flush else 0, vp(ns)),
                               keep=(keep, start, off, a, b, ns))       # (the arrays behind the addresses)

    def encode_chained_pac(self, pcm_left, pcm_right, shapes, use_huffman=True, with_flush=True, num_samples=None,
                           reservoir_in=None, want_trace=False, device=None, stream=None, want_items=False):
        """mrc_encode_chained_stream_pac: stereo streams [nStreams][stride] -- int16 PCM codes or float64 signed fractions,
        each starting with its prior hop -- + the block shapes of every stream -> the `.pac` bytes of every stream (with
        num_samples: complete files, header included), the bit reservoir carried from block to block on the device.
        pcm_right None: MONO streams (one chunk per block, one Close() chunk, nChannels = 1 in the header).
        device = (left_ptr, right_ptr or None, sample_format, stride, out_ptr, out_cap): everything stays in HBM
        (mrc_dev_encode_chained_pac; `bytes` is then None).
        -> dict: bytes (uint8), stream_offset [nStreams + 1], reservoir_out [nStreams], total, (trace), and with want_items
        item_offset [nItems + 1]: where every block's bytes start (costs a read-back of all chunk positions)."""
        q = self._chain_args(pcm_left, pcm_right, shapes, use_huffman, with_flush, num_samples, device)
        n_streams = q.n_streams
        res_in = _reservoir(reservoir_in, n_streams)
        s_off = np.zeros(n_streams + 1, np.int64)
        i_off = np.zeros(q.n_items + 1, np.int64) if want_items else None
        res_out = np.zeros(n_streams, np.int32)
        trace = np.zeros(q.n_items, np.int32) if want_trace else None
        total = np.zeros(1, np.int64)
        sched = q.head + (_p(res_in, _i32p),) + q.opts
        tail = (_p(s_off, _i64p), _p(i_off, _i64p), _p(res_out, _i32p), _p(trace, _i32p), _p(total, _i64p))
        buf = None
        if device is not None:
            self._check(lib.mrc_dev_encode_chained_pac(self._h, n_streams, *q.pcm, *sched, device[4], int(device[5]), *tail,
                                                       stream))
        else:
            bound = q.bound()
            # a buffer for typical content (~3 bits per sample); if the streams pack to more, the call says how much and
            # its bytes -- complete in the handle's device buffer -- are fetched into a buffer of that size (no second encode)
            cap = min(bound, q.n_blocks * 1024 + n_streams * 4096 + 4096)
            buf = np.empty(max(cap, 1), np.uint8)
            rc = lib.mrc_encode_chained_stream_pac(self._h, n_streams, *q.pcm, *sched, vp(buf), buf.size, *tail)
            if rc == MRC_ERR_NOMEM and 0 < int(total[0]) <= bound:
                buf = np.empty(int(total[0]), np.uint8)
                if lib.mrc_chain_fetch_output(self._h, vp(buf), buf.size, _p(total, _i64p)) != 0:
                    # a call of several slabs keeps only its last slab on the device: encode again into a buffer of the
                    # size the first pass reported
                    self._check(lib.mrc_encode_chained_stream_pac(self._h, n_streams, *q.pcm, *sched, vp(buf), buf.size, *tail))
            else:
                self._check(rc)
            buf = buf[:int(total[0])]
        out = {"bytes": buf, "stream_offset": s_off, "item_offset": i_off, "reservoir_out": res_out, "total": int(total[0])}
        if want_trace:
            out["reservoir_trace"] = trace
        return out

    def encode_chained_pac_ladder(self, pcm_left, pcm_right, shapes, rates, use_huffman=True, with_flush=True,
                                  num_samples=None, reservoir_in=None, want_trace=False, device=None, stream=None,
                                  want_items=False):
        """mrc_encode_chained_ladder_pac: encode_chained_pac at every target bit rate of `rates` (bits per sample) in ONE
        call -- phase A once, the serial scan per (rate, stream).  Result r is what encode_chained_pac gives on a handle with
        target_bits_per_sample = rates[r]; the handle's own rate is not used.  reservoir_in: None or [nRates][nStreams].
        device = (left_ptr, right_ptr or None, sample_format, stride, out_ptrs [nRates], out_caps [nRates]): PCM and outputs
        in HBM (mrc_dev_encode_chained_ladder_pac; `bytes` is then None).
        -> list of nRates dicts shaped like encode_chained_pac's."""
        rates = np.ascontiguousarray(np.atleast_1d(np.asarray(rates, dtype=np.float64)))
        R = rates.size
        q = self._chain_args(pcm_left, pcm_right, shapes, use_huffman, with_flush, num_samples, device)
        n_streams = q.n_streams
        res_in = None
        if reservoir_in is not None:
            res_in = _i32(np.asarray(reservoir_in))
            if res_in.shape != (R, n_streams):
                raise ValueError("reservoir_in must be [nRates][nStreams] = [%d][%d], got %s" % (R, n_streams, res_in.shape))
        s_off = np.zeros((R, n_streams + 1), np.int64)
        i_off = np.zeros((R, q.n_items + 1), np.int64) if want_items else None
        res_out = np.zeros((R, n_streams), np.int32)
        trace = np.zeros((R, q.n_items), np.int32) if want_trace else None
        total = np.zeros(R, np.int64)
        sched = q.head + (_p(res_in, _i32p),) + q.opts
        tail = (_p(s_off, _i64p), _p(i_off, _i64p), _p(res_out, _i32p), _p(trace, _i32p), _p(total, _i64p))
        bufs = None
        if device is not None:
            douts, dcaps = device[4], device[5]
            ptrs = (C.c_void_p * R)(*[int(p) if p else None for p in douts])
            caps = np.ascontiguousarray(dcaps, dtype=np.int64)
            if len(douts) != R or caps.shape != (R,):
                raise ValueError("device: one output pointer and one capacity per rate")
            self._check(lib.mrc_dev_encode_chained_ladder_pac(self._h, R, _p(rates, _f64p), n_streams, *q.pcm, *sched,
                                                              C.cast(ptrs, C.c_void_p), _p(caps, _i64p), *tail, stream))
        else:
            bound = q.bound()
            # a buffer per rate for typical content (1.5x the rate's bits for a long block, at least 1 KB per block); if a rate
            # packs to more, the call says how much and runs again with buffers of the reported sizes (a ladder keeps no
            # output on the device)
            per_block = [max(1024, int(1.5 * r * q.nch * 1024 / 8)) for r in rates]
            bufs = [np.empty(max(min(bound, q.n_blocks * pb + n_streams * 4096 + 4096), 1), np.uint8) for pb in per_block]
            for attempt in range(2):
                ptrs = (C.c_void_p * R)(*[buf.ctypes.data for buf in bufs])
                caps = np.array([buf.size for buf in bufs], np.int64)
                rc = lib.mrc_encode_chained_ladder_pac(self._h, R, _p(rates, _f64p), n_streams, *q.pcm, *sched,
                                                       C.cast(ptrs, C.c_void_p), _p(caps, _i64p), *tail)
                if rc == MRC_ERR_NOMEM and attempt == 0 and 0 < int(total.max()) and int(total.max()) <= bound:
                    bufs = [buf if int(t) <= buf.size else np.empty(int(t), np.uint8) for buf, t in zip(bufs, total)]
                    continue
                self._check(rc)
                break
            bufs = [buf[:int(t)] for buf, t in zip(bufs, total)]
        out = []
        for r in range(R):
            d = {"bytes": None if bufs is None else bufs[r], "stream_offset": s_off[r], "item_offset": None if i_off is None else i_off[r],
                 "reservoir_out": res_out[r], "total": int(total[r])}
            if want_trace:
                d["reservoir_trace"] = trace[r]
            out.append(d)
        return out

    # ---- what the calls that measure their own output share: the preamble, the host buffer, the per-stream dicts

    def _measured_begin(self, name, pcm_left, pcm_right, shapes, use_huffman, num_samples, device, rungs=None):
        """The preamble (name: the method, for its errors) -> the call's state: q (_chain_args), n streams, m = max(n, 1)
        (the length of a per-stream output array), the outputs every such call has -- s_off, total, and the NMR values
        tot, mx, dist ([rungs][m] with rungs, else [m]) and nblk -- and the C arguments `common` (n_streams .. num_samples)
        and `nmr_tail` (nmr_total_db .. total_bytes)."""
        if num_samples is None:
            raise ValueError("%s: num_samples is required (whole files only)" % name)
        if device is None and np.atleast_2d(pcm_left).dtype != np.int16:
            raise ValueError("%s: int16 PCM codes only (the NMR's source is int16)" % name)
        dev5 = None if device is None else (device[0], device[1], 1, device[2])
        q = self._chain_args(pcm_left, pcm_right, shapes, use_huffman, True, num_samples, dev5)
        n, m = q.n_streams, max(q.n_streams, 1)
        rows = (m,) if rungs is None else (rungs, m)
        o = SimpleNamespace(q=q, n=n, m=m, rungs=rungs, s_off=np.zeros(n + 1, np.int64), total=np.zeros(1, np.int64),
                            tot=np.zeros(rows, np.float64), mx=np.zeros(rows, np.float64), dist=np.zeros(rows, np.int64),
                            nblk=np.zeros(m, np.int64))
        o.common = (n, q.pcm[0], q.pcm[1], q.pcm[3]) + q.head + (q.opts[0], q.opts[2])
        o.nmr_tail = (_p(o.tot, _f64p), _p(o.mx, _f64p), _p(o.dist, _i64p), _p(o.nblk, _i64p), _p(o.total, _i64p))
        return o

    def _measured_call(self, cname, head, tail, o, device, stream, out_cap, typical=None, encode_again=True):
        """mrc_dev_<cname> on the caller's device buffer (-> None), or mrc_<cname> into a host buffer of out_cap bytes (None:
        the call's bound, or `typical` if that is less) -> the bytes.  If they do not fit they are fetched from the handle's
        device buffer; a call of several slabs keeps nothing there and, with encode_again, runs once more into a buffer of
        the reported size."""
        if device is not None:
            self._check(getattr(lib, "mrc_dev_" + cname)(*head, device[3], int(device[4]), *tail, stream))
            return None
        call, bound = getattr(lib, "mrc_" + cname), o.q.bound()
        if out_cap is None:
            out_cap = bound if typical is None else min(bound, typical)
        buf = np.empty(max(int(out_cap), 1), np.uint8)
        rc = call(*head, vp(buf), int(out_cap), *tail)
        if rc == MRC_ERR_NOMEM and 0 < int(o.total[0]) <= bound:
            buf = np.empty(int(o.total[0]), np.uint8)
            rc = lib.mrc_chain_fetch_output(self._h, vp(buf), buf.size, _p(o.total, _i64p))
            if rc != 0 and encode_again:
                rc = call(*head, vp(buf), buf.size, *tail)
        self._check(rc)
        return buf

    @staticmethod
    def _measured_results(o, buf, **own):
        """-> one dict per stream: data (the stream's bytes; (start, end) in the caller's buffer if buf is None), the call's
        own fields (a list with an entry per stream each), the NMR fields.  Columns are converted once, not per stream."""
        n, off = o.n, o.s_off.tolist()
        data = [(off[s], off[s + 1]) if buf is None else buf[off[s]:off[s + 1]].tobytes() for s in range(n)]
        if o.rungs is None:
            nmr = [o.tot[:n].tolist(), o.mx[:n].tolist(), o.dist[:n].tolist()]
        else:
            nmr = [[a[:, s].copy() for s in range(n)] for a in (o.tot, o.mx, o.dist)]
        keys = ("data",) + tuple(own) + ("nmr_total_db", "nmr_max_db", "disturbed_blocks", "n_blocks")
        return [dict(zip(keys, row)) for row in zip(data, *own.values(), *nmr, o.nblk[:n].tolist())]

    def encode_chained_pac_target_nmr(self, pcm_left, pcm_right, shapes, rates, target_db, use_huffman=True, num_samples=None,
                                      device=None, stream=None, out_cap=None):
        """mrc_encode_chained_target_nmr_pac: the streams of encode_chained_pac_ladder (int16 PCM codes, each row starting
        with its zero prior hop) at every rate of `rates` (strictly ascending), the noise-to-mask ratio of every rung measured
        on the device, and per stream the complete `.pac` file of the LOWEST rung whose nmr_total_db is <= target_db (the top
        rung, met False, if none is).  num_samples [nStreams] is required: whole files only.
        device = (left_ptr, right_ptr or None, stride, out_ptr, out_cap): PCM and output in HBM
        (mrc_dev_encode_chained_target_nmr_pac; `data` is then the (start, end) bytes of the stream's file in out).
        out_cap: the size of the host buffer (default: sized for typical content, fetched from the device if too small).
        -> one dict per stream: data (bytes), chosen, rate, met, nmr_total_db [R], nmr_max_db [R], disturbed_blocks [R],
        n_blocks -- the numbers pac_nmr gives for every rung's file."""
        rates = np.ascontiguousarray(np.atleast_1d(np.asarray(rates, dtype=np.float64)))
        o = self._measured_begin("encode_chained_pac_target_nmr", pcm_left, pcm_right, shapes, use_huffman, num_samples, device,
                                 rungs=rates.size)
        chosen, met = np.zeros(o.m, np.int32), np.zeros(o.m, np.int32)
        head = (self._h, rates.size, _p(rates, _f64p), float(target_db)) + o.common
        tail = (_p(o.s_off, _i64p), _p(chosen, _i32p), _p(met, _i32p)) + o.nmr_tail
        # typical content at the top rate; more: fetched from TargetBufs::sel, which holds the whole result (no second encode)
        typical = None
        if device is None and out_cap is None:
            typical = o.q.n_blocks * max(1024, int(1.5 * rates.max() * o.q.nch * 1024 / 8)) + o.n * 4096 + 4096
        buf = self._measured_call("encode_chained_target_nmr_pac", head, tail, o, device, stream, out_cap, typical,
                                  encode_again=False)
        chosen = chosen[:o.n]
        return self._measured_results(o, buf, chosen=chosen.tolist(), rate=rates[chosen].tolist(),
                                      met=met[:o.n].astype(bool).tolist())

    def target_ms(self):
        """device time of the last encode_chained_pac_target_nmr: phase A + preparation, serial scan, NMR kernels
        (threshold pass included), pack + gather (ms)"""
        ms = np.zeros(4, np.float64)
        self._check(lib.mrc_get_target_ms(self._h, _p(ms, _f64p)))
        return ms

    def encode_vbr_nmr_pac(self, pcm_left, pcm_right, shapes, ceiling_db, use_huffman=True, num_samples=None, device=None,
                           stream=None, out_cap=None):
        """mrc_encode_vbr_nmr_pac: constant-quality VBR.  The streams of encode_chained_pac (int16 PCM codes, each row
        starting with its zero prior hop) coded without a bit budget: every band of every block gets the fewest mantissa
        bits at which its measured noise-to-mask ratio is <= 10^(ceiling_db / 10).  num_samples [nStreams] is required:
        whole files only.
        device = (left_ptr, right_ptr or None, stride, out_ptr, out_cap): PCM and output in HBM (mrc_dev_encode_vbr_nmr_pac;
        `data` is then the (start, end) bytes of the stream's file in out).
        out_cap: the size of the host buffer (default: the call's bound).
        -> one dict per stream: data (bytes), ceiling_ratio, capped_bands, coded_bits, nmr_total_db, nmr_max_db,
        disturbed_blocks, n_blocks -- the numbers pac_nmr gives for the file."""
        o = self._measured_begin("encode_vbr_nmr_pac", pcm_left, pcm_right, shapes, use_huffman, num_samples, device)
        ratio, capped, bits = np.zeros(1, np.float64), np.zeros(o.m, np.int64), np.zeros(o.m, np.int64)
        head = (self._h, float(ceiling_db)) + o.common
        tail = (_p(o.s_off, _i64p), _p(ratio, _f64p), _p(capped, _i64p), _p(bits, _i64p)) + o.nmr_tail
        buf = self._measured_call("encode_vbr_nmr_pac", head, tail, o, device, stream, out_cap)
        return self._measured_results(o, buf, ceiling_ratio=[float(ratio[0])] * o.n, capped_bands=capped[:o.n].tolist(),
                                      coded_bits=bits[:o.n].tolist())

    def vbr_ms(self):
        """device time of the last encode_vbr_nmr_pac: phase A + source analysis, the allocator, pack, their sum (ms)"""
        ms = np.zeros(4, np.float64)
        self._check(lib.mrc_get_vbr_ms(self._h, _p(ms, _f64p)))
        return ms

    def encode_vbr_size_pac(self, pcm_left, pcm_right, shapes, target_bytes, lo_db=-30.0, step_db=0.25, n=256, use_huffman=True,
                            num_samples=None, device=None, stream=None, out_cap=None):
        """mrc_encode_vbr_size_pac: constant-quality VBR to a file size.  The streams of encode_vbr_nmr_pac, each coded at the
        tightest ceiling of the grid lo_db + i * step_db (i < n) that the bisection of pacfile.bisect_ceiling finds to fit
        target_bytes [nStreams] (the complete file).  device / out_cap as in encode_vbr_nmr_pac.
        -> one dict per stream: encode_vbr_nmr_pac's at the chosen ceiling plus chosen, chosen_db, met, probes, probe_index
        and probe_bytes (the grid index and file size of every probe in order)."""
        o = self._measured_begin("encode_vbr_size_pac", pcm_left, pcm_right, shapes, use_huffman, num_samples, device)
        ns, m = o.n, o.m
        target = np.ascontiguousarray(target_bytes, dtype=np.int64).reshape(-1)
        if target.shape != (ns,):
            raise ValueError("target_bytes: one value per stream")
        chosen, met, probes = np.zeros(m, np.int32), np.zeros(m, np.int32), np.zeros(m, np.int32)
        chosen_db, ratio = np.zeros(m, np.float64), np.zeros(m, np.float64)
        p_idx, p_bytes = np.full((m, MRC_MAX_PROBES), -1, np.int32), np.full((m, MRC_MAX_PROBES), -1, np.int64)
        capped, bits = np.zeros(m, np.int64), np.zeros(m, np.int64)
        head = (self._h, float(lo_db), float(step_db), int(n), _p(target, _i64p)) + o.common
        tail = (_p(o.s_off, _i64p), _p(chosen, _i32p), _p(chosen_db, _f64p), _p(ratio, _f64p), _p(met, _i32p), _p(probes, _i32p),
                _p(p_idx, _i32p), _p(p_bytes, _i64p), _p(capped, _i64p), _p(bits, _i64p)) + o.nmr_tail
        buf = self._measured_call("encode_vbr_size_pac", head, tail, o, device, stream, out_cap)
        k = probes[:ns].tolist()
        return self._measured_results(
            o, buf, chosen=chosen[:ns].tolist(), chosen_db=chosen_db[:ns].tolist(), ceiling_ratio=ratio[:ns].tolist(),
            met=met[:ns].astype(bool).tolist(), probes=k, probe_index=[row[:c] for row, c in zip(p_idx.tolist(), k)],
            probe_bytes=[row[:c] for row, c in zip(p_bytes.tolist(), k)], capped_bands=capped[:ns].tolist(),
            coded_bits=bits[:ns].tolist())

    def vbr_size_ms(self):
        """device time of the last encode_vbr_size_pac: phase A + source analysis, the profile kernel, all probes, the final
        pick + pack, their sum (ms)"""
        ms = np.zeros(5, np.float64)
        self._check(lib.mrc_get_vbr_size_ms(self._h, _p(ms, _f64p)))
        return ms

    def chain_out_bound(self, block_start, block_a, block_b, with_flush=True, with_headers=True, n_channels=2):
        """mrc_chain_out_bound_ex: the worst-case output bytes of a chained call on n_channels = 1 (mono) or 2 streams."""
        start = np.ascontiguousarray(block_start, dtype=np.int64)
        a, b = np.ascontiguousarray(block_a, dtype=np.int32), np.ascontiguousarray(block_b, dtype=np.int32)
        return int(lib.mrc_chain_out_bound_ex(self._h, int(n_channels), len(start) - 1, _p(start, _i64p), _p(a, _i32p),
                                              _p(b, _i32p), 1 if with_flush else 0, 1 if with_headers else 0))

    def chain_ms(self):
        """device time of the last chained encode: phase A + preparation, serial scan, packing, all three (ms)"""
        ms = np.zeros(4, np.float64)
        self._check(lib.mrc_get_chain_ms(self._h, _p(ms, _f64p)))
        return ms

    def pcm_to_float(self, pcm):
        pcm = np.ascontiguousarray(pcm, dtype=np.int16)
        out = np.empty(pcm.shape, np.float64)
        self._check(lib.mrc_pcm_to_float(self._h, pcm.size, pcm.ctypes.data_as(C.c_void_p), _p(out, _f64p)))
        return out

    def quantize_uniform(self, x, n_bits):
        x = _f64(np.atleast_1d(x))
        out = np.empty(x.shape, np.int64)
        self._check(lib.mrc_quantize_uniform(self._h, x.size, int(n_bits), _p(x, _f64p), _p(out, _i64p)))
        return out

    def bark(self, f):
        f = _f64(np.atleast_1d(f))
        out = np.empty(f.shape, np.float64)
        self._check(lib.mrc_bark(self._h, f.size, _p(f, _f64p), _p(out, _f64p)))
        return out

    def window(self, blocks, a, b):
        blocks = _f64(blocks)
        out = np.empty_like(blocks)
        self._check(lib.mrc_window(self._h, blocks.shape[0], a, b, _p(blocks, _f64p), _p(out, _f64p)))
        return out

    def mdct(self, blocks, a, b, apply_window=True):
        blocks = _f64(blocks)
        n = blocks.shape[0]
        lines = np.empty((n, (a + b) // 2), np.float64)
        scale = np.empty(n, np.int32)
        self._check(lib.mrc_mdct(self._h, n, a, b, _p(blocks, _f64p), int(bool(apply_window)), _p(lines, _f64p),
                                 _p(scale, _i32p)))
        return lines, scale

    def smr(self, blocks, a, b, scaled_lines=None, overall_scale=None, want_thresh=False):
        blocks = _f64(blocks)
        n = blocks.shape[0]
        nb, half = len(self.bands(a, b)), (a + b) // 2
        smr = np.empty((n, nb), np.float64)
        thr = np.empty((n, half), np.float64) if want_thresh else None
        sl = None if scaled_lines is None else _f64(scaled_lines)
        sc = None if overall_scale is None else _i32(overall_scale)
        self._check(lib.mrc_smr(self._h, n, a, b, _p(blocks, _f64p), _p(sl, _f64p), _p(sc, _i32p), _p(smr, _f64p),
                                _p(thr, _f64p)))
        return (smr, thr) if want_thresh else smr

    def bitalloc(self, budget, max_mant_bits, n_lines, smr, want_smr_after=False):
        """-> (bits [n][nb], bits_left [n]) and, with want_smr_after, the running SMRs the loop leaves behind
        (bitalloc.py:132-151 updates its SMR argument in place)."""
        smr = _f64(np.atleast_2d(smr))
        n, nb = smr.shape
        budget = _f64(np.broadcast_to(np.asarray(budget, dtype=np.float64), (n,)))
        nl = _i32(n_lines)
        bits = np.empty((n, nb), np.int32)
        left = np.empty(n, np.int32)
        if want_smr_after:
            after = smr.copy()
            self._check(lib.mrc_bitalloc_inplace(self._h, n, nb, int(max_mant_bits), _p(nl, _i32p), _p(budget, _f64p),
                                                 _p(after, _f64p), _p(bits, _i32p), _p(left, _i32p)))
            return bits, left, after
        self._check(lib.mrc_bitalloc(self._h, n, nb, int(max_mant_bits), _p(nl, _i32p), _p(budget, _f64p),
                                     _p(smr, _f64p), _p(bits, _i32p), _p(left, _i32p)))
        return bits, left

    def scale_factor(self, v, n_scale_bits, n_mant_bits):
        v = _f64(np.atleast_1d(v))
        mb = _i32(np.broadcast_to(np.asarray(n_mant_bits), v.shape))
        out = np.empty(v.shape, np.int32)
        self._check(lib.mrc_scale_factor(self._h, v.size, int(n_scale_bits), _p(v, _f64p), _p(mb, _i32p),
                                         _p(out, _i32p)))
        return out

    def mantissa(self, x, scale, n_scale_bits, n_mant_bits):
        x = _f64(np.atleast_1d(x))
        sc = _i32(np.broadcast_to(np.asarray(scale), x.shape))
        mb = _i32(np.broadcast_to(np.asarray(n_mant_bits), x.shape))
        out = np.empty(x.shape, np.int32)
        self._check(lib.mrc_mantissa(self._h, x.size, int(n_scale_bits), _p(x, _f64p), _p(sc, _i32p), _p(mb, _i32p),
                                     _p(out, _i32p)))
        return out

    def huffman_gain(self, bit_alloc, mantissa, a, b):
        """bit_alloc [n][nStreams][nBands], mantissa [n][nStreams][N/2] dense -> (table id [n][nStreams], bits_saved)."""
        ba, m = _i32(bit_alloc), _i32(mantissa)
        n, ns = ba.shape[0], ba.shape[1]
        table = np.empty((n, ns), np.int32)
        saved = np.empty((n, ns), np.int32)
        self._check(lib.mrc_huffman_gain(self._h, n, int(a), int(b), ns, _p(ba, _i32p), _p(m, _i32p), _p(table, _i32p),
                                         _p(saved, _i32p)))
        return table, saved

    def dev_huffman_gain(self, a, b, n_frames, n_streams, bit_alloc, mantissa, reservoir_out, huff_table, bits_saved,
                         reservoir_next=None, stream=None):
        self._check(lib.mrc_dev_huffman_gain(self._h, a, b, n_frames, n_streams, bit_alloc, mantissa, reservoir_out,
                                             huff_table, bits_saved, reservoir_next, stream))

    def dev_pack_blocks(self, a, b, n_blocks, n_channels, joint, use_huffman, huff_table_in, overall_scale, ms_switch,
                        scale_factor, bit_alloc, mantissa, mantissa16, out, out_cap, block_offset, huff_table=None,
                        bits_saved=None, want_total=True, stream=None):
        """`.pac` chunks packed on the device (mrc_dev_pack_blocks): every array argument is a DEVICE address.  -> total
        bytes (want_total: waits for the stream), else None."""
        total = np.zeros(1, np.int64)
        self._check(lib.mrc_dev_pack_blocks(self._h, a, b, n_blocks, n_channels, 1 if joint else 0, 1 if use_huffman else 0,
                                            huff_table_in, overall_scale, ms_switch, scale_factor, bit_alloc, mantissa,
                                            1 if mantissa16 else 0, out, out_cap, block_offset, huff_table, bits_saved,
                                            total.ctypes.data_as(_i64p) if want_total else None, stream))
        return int(total[0]) if want_total else None

    # ---- decode side
    def decode(self, a, b, overall_scale, scale_factor, bit_alloc, mantissa, ms_switch=None):
        """codecThem.Decode / JointDecode for n blocks of shape (a,b): scale_factor / bit_alloc [n][nStreams][nBands],
        mantissa [n][nStreams][N/2] dense, overall_scale [n] (mono) or [n][4] with ms_switch [n][nBands] (joint)
        -> windowed blocks [n][nStreams][a+b] (before overlap-and-add)."""
        sf, ba, m, osc = _i32(scale_factor), _i32(bit_alloc), _i32(mantissa), _i32(overall_scale)
        n, ns = sf.shape[0], sf.shape[1]
        nb, half = len(self.bands(a, b)), (a + b) // 2
        if sf.shape != (n, ns, nb) or ba.shape != sf.shape or m.shape != (n, ns, half) or ns not in (1, 2):
            raise ValueError("decode: array shapes do not match the block shape")
        sw = None
        if ns == 2:
            sw = _i32(ms_switch)
            if sw.shape != (n, nb) or osc.shape != (n, 4):
                raise ValueError("decode: joint blocks need overall_scale [n][4] and ms_switch [n][nBands]")
        elif osc.size != n:
            raise ValueError("decode: overall_scale [n] expected")
        out = np.empty((n, ns, a + b), np.float64)
        self._check(lib.mrc_decode(self._h, n, int(a), int(b), ns, _p(osc, _i32p), _p(sw, _i32p), _p(sf, _i32p),
                                   _p(ba, _i32p), _p(m, _i32p), _p(out, _f64p)))
        return out

    def pcm16(self, x):
        x = _f64(x)
        out = np.empty(x.shape, np.int16)
        self._check(lib.mrc_pcm16(self._h, x.size, _p(x, _f64p), out.ctypes.data_as(C.POINTER(C.c_int16))))
        return out

    def dev_decode(self, a, b, n_blocks, n_streams, overall_scale, ms_switch, scale_factor, bit_alloc, mantissa,
                   out_offset, out_left, out_right=None, stream=None):
        self._check(lib.mrc_dev_decode(self._h, a, b, n_blocks, n_streams, overall_scale, ms_switch, scale_factor,
                                       bit_alloc, mantissa, out_offset, out_left, out_right, stream))

    def dev_pcm16(self, n, x, out, stream=None):
        self._check(lib.mrc_dev_pcm16(self._h, n, x, out, stream))

    def dev_unpack_blocks(self, n_blocks, n_channels, joint, buf, length, chunk_offset, a, b, huff_table, overall_scale,
                          ms_switch, scale_factor, bit_alloc, mantissa, stream=None):
        """mrc_dev_unpack_blocks: the chunk parser of pacfile.unpack_blocks on the device, same fixed-stride layout; every
        array argument is a DEVICE address.  Waits for the stream; a chunk the host parser would refuse raises MrcError."""
        self._check(lib.mrc_dev_unpack_blocks(self._h, int(n_blocks), int(n_channels), 1 if joint else 0, buf, int(length),
                                              chunk_offset, a, b, huff_table, overall_scale, ms_switch, scale_factor,
                                              bit_alloc, mantissa, stream))

    def decode_pac_pcm16(self, bufs, interleaved=True):
        """mrc_decode_pac_pcm16: whole `.pac` files (bytes-like, one or a list) -> 16-bit PCM, parsed and decoded on the
        device in one call.  Returns a list with one int16 array per file: [samples][nCh] in WAV order (views of one
        interleaved buffer) or, interleaved=False, [nCh][samples] as pacfile.decode_pac_pcm16 returns it."""
        if isinstance(bufs, (bytes, bytearray, memoryview, np.ndarray)):
            bufs = [bufs]
        n = len(bufs)
        sizes = np.fromiter((len(b) for b in bufs), dtype=np.int64, count=n)
        file_offset = np.zeros(n + 1, np.int64)
        np.cumsum(sizes, out=file_offset[1:])
        if n == 1:
            data = np.ascontiguousarray(np.frombuffer(bufs[0], np.uint8))
        else:
            data = np.frombuffer(b"".join(bytes(b) for b in bufs), np.uint8)
        sample_offset = np.zeros(n + 1, np.int64)
        nch = np.zeros(max(n, 1), np.int32)
        # a first guess (typical files code ~3 bits per sample); a short one costs only the host's header / chunk scan
        out = np.empty(6 * data.size + 4096, np.int16)
        args = lambda o: (self._h, n, _p(data, _u8p), _p(file_offset, _i64p), o.ctypes.data_as(C.c_void_p), o.size,
                          _p(sample_offset, _i64p), _p(nch, _i32p))
        rc = lib.mrc_decode_pac_pcm16(*args(out))
        if rc == MRC_ERR_NOMEM and int(sample_offset[n]) > out.size:
            out = np.empty(int(sample_offset[n]), np.int16)
            rc = lib.mrc_decode_pac_pcm16(*args(out))
        self._check(rc)
        res = []
        for f in range(n):
            v = out[sample_offset[f]:sample_offset[f + 1]].reshape(-1, int(nch[f]))
            res.append(v if interleaved else v.T)
        return res

    def decode_ms(self):
        """device time of the last decode_pac_pcm16: H2D copy, unpack, synthesis (decode + pcm16), D2H copy (ms)"""
        ms = np.zeros(4, np.float64)
        self._check(lib.mrc_get_decode_ms(self._h, _p(ms, _f64p)))
        return ms

    def pac_nmr(self, bufs, sources, detail=False):
        """mrc_pac_nmr: the noise-to-mask ratio of whole `.pac` files (bytes-like, one or a list) against their sources,
        one int16 [nCh][n] array per file (the WAV's own samples, no prior hop; the same object may repeat and is then
        uploaded once).  Returns one dict per file: nmr_max_db, nmr_total_db, disturbed_blocks, n_blocks; with
        detail=True also shape [E, 2] (a, b per entry: block, then channel), noise and mask [E, nBands of the widest
        block] and nmr_db = 10 log10(noise / mask) (0 ratio where mask is +inf), NaN past a block's bands."""
        if isinstance(bufs, (bytes, bytearray, memoryview, np.ndarray)):
            bufs = [bufs]
            sources = [sources]
        data, file_offset, src, src_offset, src_stride, src_frames, n_entries = nmr_layout(bufs, sources)
        n = len(bufs)
        mx, tot = np.zeros(max(n, 1)), np.zeros(max(n, 1))
        dist, nblk = np.zeros(max(n, 1), np.int64), np.zeros(max(n, 1), np.int64)
        entry_offset = np.zeros(n + 1, np.int64)
        cap = 0
        shape = noise = mask = None

        def call():
            return lib.mrc_pac_nmr(self._h, n, _p(data, _u8p), _p(file_offset, _i64p), src.ctypes.data_as(C.c_void_p),
                                   _p(src_offset, _i64p), _p(src_stride, _i64p), _p(src_frames, _i64p), _p(mx, _f64p),
                                   _p(tot, _f64p), _p(dist, _i64p), _p(nblk, _i64p), _p(entry_offset, _i64p), cap,
                                   _p(shape, _i32p), _p(noise, _f64p), _p(mask, _f64p))
        if detail:
            cap = max(1, n_entries)                # one entry per chunk (exact unless a file is refused)
            shape = np.zeros((cap, 2), np.int32)
            noise, mask = np.zeros((cap, MRC_MAX_BANDS)), np.zeros((cap, MRC_MAX_BANDS))
        rc = call()
        if detail and rc == MRC_ERR_NOMEM and int(entry_offset[n]) > cap:
            cap = int(entry_offset[n])
            shape = np.zeros((cap, 2), np.int32)
            noise, mask = np.zeros((cap, MRC_MAX_BANDS)), np.zeros((cap, MRC_MAX_BANDS))
            rc = call()
        self._check(rc)
        res = []
        for f in range(n):
            r = dict(nmr_max_db=float(mx[f]), nmr_total_db=float(tot[f]), disturbed_blocks=int(dist[f]),
                     n_blocks=int(nblk[f]))
            if detail:
                e0, e1 = int(entry_offset[f]), int(entry_offset[f + 1])
                sh = shape[e0:e1].copy()
                keys = sh[:, 0].astype(np.int64) * 65536 + sh[:, 1]
                uk, inv = np.unique(keys, return_inverse=True)
                nbands = np.array([len(self.bands(int(k) // 65536, int(k) % 65536)) for k in uk], np.int64)[inv.reshape(-1)]
                w = int(nbands.max()) if e1 > e0 else 0
                no, ma = noise[e0:e1, :w].copy(), mask[e0:e1, :w].copy()
                with np.errstate(divide="ignore", invalid="ignore"):
                    ratio = np.where(np.isinf(ma), 0.0, no / ma)
                    db = 10.0 * np.log10(ratio)
                past = np.arange(w)[None, :] >= nbands[:, None]
                for a in (no, ma, db):
                    a[past] = np.nan
                r.update(shape=sh, noise=no, mask=ma, nmr_db=db)
            res.append(r)
        return res

    def nmr_ms(self):
        """device time of the last pac_nmr: H2D copy, unpack, source analysis, NMR kernels + D2H copy (ms)"""
        ms = np.zeros(4, np.float64)
        self._check(lib.mrc_get_nmr_ms(self._h, _p(ms, _f64p)))
        return ms

    def transient_peaks(self, streams, sos):
        """streams [nCh][(nHops+1)*hop], float64 signed fractions or the file's int16 PCM codes -> peaks
        [nHops][nCh][hop/nShort + 1] (sub-block peaks, then the hop's peak)."""
        x = np.atleast_2d(streams)
        fmt = 1 if x.dtype == np.int16 else 0
        x = np.ascontiguousarray(x, dtype=np.int16 if fmt else np.float64)
        sos = _f64(sos)
        hop, n_short = self.cfg.n_mdct_lines, self.cfg.n_short
        n_hops = x.shape[1] // hop - 1
        if x.shape[1] != (n_hops + 1) * hop or sos.ndim != 2 or sos.shape[1] != 6:
            raise ValueError("streams must be [nCh][(nHops+1)*hop], sos [nSections][6]")
        out = np.empty((max(n_hops, 0), x.shape[0], hop // n_short + 1), np.float64)
        self._check(lib.mrc_transient_peaks_ex(self._h, n_hops, x.shape[0], sos.shape[0], _p(sos, _f64p),
                                               x.ctypes.data_as(C.c_void_p), fmt, _p(out, _f64p)))
        return out

    def dev_transient_peaks(self, n_hops, n_channels, sos, streams_ptr, sample_format, channel_stride, peaks_ptr, stream=None):
        """mrc_dev_transient_peaks: streams / peaks are device addresses, sos a host array [nSections][6]."""
        sos = _f64(sos)
        self._check(lib.mrc_dev_transient_peaks(self._h, int(n_hops), int(n_channels), sos.shape[0], _p(sos, _f64p), streams_ptr,
                                                int(sample_format), int(channel_stride), peaks_ptr, stream))

    def stereo_masking_factor(self, mid_thresh, side_thresh, z):
        m, s_, zz = _f64(mid_thresh), _f64(side_thresh), _f64(z)
        if not (m.shape == s_.shape == zz.shape):
            raise ValueError("mid, side and z must have the same shape")
        om, os_ = np.empty_like(m), np.empty_like(m)
        self._check(lib.mrc_stereo_masking_factor(self._h, m.size, _p(m, _f64p), _p(s_, _f64p), _p(zz, _f64p),
                                                  _p(om, _f64p), _p(os_, _f64p)))
        return om, os_

    def ms_switch(self, lines_left, lines_right, n_lines):
        L, R = _f64(np.atleast_2d(lines_left)), _f64(np.atleast_2d(lines_right))
        nl = _i32(n_lines)
        if L.shape != R.shape or L.shape[1] != int(nl.sum()):
            raise ValueError("line vectors must be [n][sum(n_lines)]")
        out = np.empty((L.shape[0], len(nl)), np.int32)
        self._check(lib.mrc_ms_switch(self._h, L.shape[0], len(nl), _p(nl, _i32p), _p(L, _f64p), _p(R, _f64p),
                                      _p(out, _i32p)))
        return out

    # ---- device entry points (raw pointers as ints, e.g. torch.Tensor.data_ptr())
    def dev_encode(self, a, b, n_frames, ch_left, ch_right, frame_stride, offsets, reservoir_in, overall_scale,
                   ms_switch, bit_alloc, scale_factor, mantissa, reservoir_out, lines_out=None, stream=None):
        self._check(lib.mrc_dev_encode(self._h, a, b, n_frames, ch_left, ch_right, frame_stride, offsets,
                                       reservoir_in, overall_scale, ms_switch, bit_alloc, scale_factor, mantissa,
                                       reservoir_out, lines_out, stream))

    def dev_encode_ex(self, a, b, n_frames, ch_left, ch_right, sample_format, frame_stride, offsets, reservoir_in,
                      overall_scale, ms_switch, bit_alloc, scale_factor, mantissa, mantissa_format, reservoir_out,
                      lines_out=None, stream=None):
        self._check(lib.mrc_dev_encode_ex(self._h, a, b, n_frames, ch_left, ch_right, int(sample_format), frame_stride,
                                          offsets, reservoir_in, overall_scale, ms_switch, bit_alloc, scale_factor,
                                          mantissa, int(mantissa_format), reservoir_out, lines_out, stream))

    def dev_mdct(self, a, b, n_frames, ch_left, ch_right, frame_stride, offsets, lines, overall_scale, stream=None):
        self._check(lib.mrc_dev_mdct(self._h, a, b, n_frames, ch_left, ch_right, frame_stride, offsets, lines,
                                     overall_scale, stream))

    def dev_smr(self, a, b, n_frames, ch_left, ch_right, frame_stride, offsets, lines, overall_scale, smr,
                thresh=None, stream=None):
        self._check(lib.mrc_dev_smr(self._h, a, b, n_frames, ch_left, ch_right, frame_stride, offsets, lines,
                                    overall_scale, smr, thresh, stream))

    def dev_masking(self, a, b, n_frames, ch_left, ch_right, sample_format, frame_stride, offsets, lines, overall_scale,
                    ms_switch, smr, band_peak, stream=None):
        self._check(lib.mrc_dev_masking(self._h, a, b, n_frames, ch_left, ch_right, int(sample_format), frame_stride,
                                        offsets, lines, overall_scale, ms_switch, smr, band_peak, stream))

    def dev_helper_probe(self, probe, in0, in1, in2, out, out_words, n, threads=64, stream=None):
        """one __device__ helper on device arrays of 8-byte words (include/mrc_hip.h: mrc_dev_helper_probe; PROBES names the
        probes and their words per element)"""
        self._check(lib.mrc_dev_helper_probe(self._h, int(probe), in0, in1, in2, out, int(out_words), int(n), int(threads),
                                             stream))

    def dev_alloc_quant(self, a, b, n_frames, joint, lines, overall_scale, smr, reservoir_in, ms_switch, bit_alloc,
                        scale_factor, mantissa, reservoir_out, stream=None):
        self._check(lib.mrc_dev_alloc_quant(self._h, a, b, n_frames, int(joint), lines, overall_scale, smr,
                                            reservoir_in, ms_switch, bit_alloc, scale_factor, mantissa,
                                            reservoir_out, stream))

    def dev_alloc_quant_chained(self, a, b, n_frames, joint, blocks_per_stream, use_huffman, lines, overall_scale, smr,
                                reservoir_in, ms_switch, bit_alloc, scale_factor, mantissa16, huff_table, reservoir_out,
                                reservoir_trace=None, stream=None):
        """mrc_dev_alloc_quant through the chained back end: streams of blocks_per_stream consecutive blocks, reservoirs
        per stream, the mantissa plane uint16"""
        self._check(lib.mrc_dev_alloc_quant_chained(self._h, a, b, n_frames, int(joint), int(blocks_per_stream),
                                                    int(bool(use_huffman)), lines, overall_scale, smr, reservoir_in,
                                                    ms_switch, bit_alloc, scale_factor, mantissa16, huff_table,
                                                    reservoir_out, reservoir_trace, stream))

    @staticmethod
    def vbr_record_width(joint):
        """ratios per band of a VBR record (dev_vbr_profile / dev_vbr_pick)"""
        return int(lib.mrc_vbr_record_width(int(bool(joint))))

    def dev_vbr_alloc(self, a, b, n_frames, joint, ceiling, lines, overall_scale, ms_switch, source_lines, source_thresh,
                      bit_alloc, scale_factor, mantissa16, stat, capped, stream=None):
        """vbr_alloc_kernel on caller-made planes at the LINEAR ceiling (include/mrc_hip.h: mrc_dev_vbr_alloc)"""
        self._check(lib.mrc_dev_vbr_alloc(self._h, a, b, n_frames, int(bool(joint)), float(ceiling), lines, overall_scale,
                                          ms_switch, source_lines, source_thresh, bit_alloc, scale_factor, mantissa16, stat,
                                          capped, stream))

    def dev_vbr_profile(self, a, b, n_frames, joint, lines, overall_scale, ms_switch, source_lines, source_thresh, ratios,
                        picks, stream=None):
        """vbr_profile_kernel on caller-made planes: the record ratios [n][nBands][vbr_record_width(joint)] (NaN where the
        walk wrote nothing) and picks [n][nBands] (joint)"""
        self._check(lib.mrc_dev_vbr_profile(self._h, a, b, n_frames, int(bool(joint)), lines, overall_scale, ms_switch,
                                            source_lines, source_thresh, ratios, picks, stream))

    def dev_vbr_pick(self, a, b, n_frames, joint, ceilings, lines, overall_scale, ms_switch, ratios, picks, bit_alloc,
                     scale_factor, mantissa16, stat, capped, stream=None):
        """vbr_pick_kernel on a record of dev_vbr_profile, one linear ceiling per block"""
        self._check(lib.mrc_dev_vbr_pick(self._h, a, b, n_frames, int(bool(joint)), ceilings, lines, overall_scale, ms_switch,
                                         ratios, picks, bit_alloc, scale_factor, mantissa16, stat, capped, stream))

    def set_option(self, option, value):
        self._check(lib.mrc_set_option(self._h, int(option), int(value)))

    def get_option(self, option):
        v = C.c_int32()
        self._check(lib.mrc_get_option(self._h, int(option), C.byref(v)))
        return v.value

    SENS_NAMES = ("quantiser_edges", "bitalloc_near_ties", "ms_switch_near_threshold", "peak_near_ties",
                  "node_chunks_sent_back", "blocks_examined")

    def sensitivity(self, reset=True):
        """mrc_get_sensitivity: with set_option(5, 1) (MRC_OPT_SENSITIVITY) the encode calls count the integer decisions
        taken within a guard band of floating-point rounding -> dict name -> count since the last reset."""
        v = np.zeros(8, np.int64)
        self._check(lib.mrc_get_sensitivity(self._h, _p(v, _i64p), 1 if reset else 0))
        return {n: int(v[i]) for i, n in enumerate(self.SENS_NAMES)}

    def set_timing(self, on):
        self._check(lib.mrc_set_timing(self._h, int(bool(on))))

    def stage_ms(self):
        ms = np.zeros(3, np.float64)
        self._check(lib.mrc_get_stage_ms(self._h, _p(ms, _f64p)))
        return ms

    def kernel_ms(self):
        """device time of the last timed encode per kernel: MDCT, smr, band_stats (joint), bitalloc, quantize"""
        ms = np.zeros(5, np.float64)
        self._check(lib.mrc_get_kernel_ms(self._h, _p(ms, _f64p)))
        return ms


MRC_SAMPLES_F64, MRC_SAMPLES_PCM16 = 0, 1
MRC_MANTISSA_I32, MRC_MANTISSA_I16 = 0, 1


class PinnedArray:
    """A NumPy array over page-locked host memory (mrc_host_alloc): what makes the copies of
    Handle.encode_stream_pcm16 asynchronous.  Keep the object alive as long as `.array` is used."""

    def __init__(self, shape, dtype):
        dt = np.dtype(dtype)
        n = int(np.prod(shape)) * dt.itemsize
        self._p = C.c_void_p()
        rc = lib.mrc_host_alloc(C.byref(self._p), max(n, 1))
        if rc != 0:
            raise MrcError("mrc_host_alloc(%d bytes) failed (%d)" % (n, rc))
        buf = (C.c_char * max(n, 1)).from_address(self._p.value)
        self.array = np.frombuffer(buf, dtype=dt, count=int(np.prod(shape))).reshape(shape)

    def free(self):
        if getattr(self, "_p", None) is not None and self._p.value:
            self.array = None
            lib.mrc_host_free(self._p)
            self._p = C.c_void_p()

    def __del__(self):
        try:
            self.free()
        except Exception:
            pass
