"""ctypes binding of libdt_hip.so (C ABI: include/dt_hip.h).  No fallback: a missing or
unloadable library raises, and every non-zero status from the library raises."""
import ctypes
import os
from ctypes import (POINTER, c_char_p, c_double, c_float, c_int, c_int32, c_int64, c_longlong, c_size_t, c_uint8,
                    c_void_p)

_LIB = None
LIB_PATH = os.path.join(os.path.dirname(os.path.abspath(__file__)), "csrc", "libdt_hip.so")

COND_NONE, COND_ZERO, COND_ONE = 0, 1, 2
RULE_ENGINE, RULE_PSAMPLE, RULE_MANAGER = 0, 1, 2
PREC_FP32, PREC_SPLIT_BF16, PREC_AUTO = 0, 1, 2
# convolution launch kinds (csrc/dt_internal.h ConvKind) as dt_unet_conv_choice reports them (+8: the block's 1x1 skip is folded
# into that conv2 launch) and dt_unet_set_conv_choice / the plan table take them
KIND_FP32 = 0
KIND_NAMES = {KIND_FP32: "fp32", 1: "split-bf16", 3: "split-bf16-strip", 4: "split-bf16-strip32", 5: "split-bf16-stripk"}
BT_COUNT, GT_COUNT, N_BLOCKS = 16, 9, 8
ABI_VERSION = 6


class HipLibraryError(RuntimeError):
    pass


class UNetDesc(ctypes.Structure):
    _fields_ = [("channels", c_int32), ("dims", c_int32 * 4), ("temb_dim", c_int32)]


# name -> (restype, argtypes); must list every symbol include/dt_hip.h declares
SIGNATURES = {
    "dt_abi_version": (c_int, []),
    "dt_status_string": (c_char_p, [c_int]),
    "dt_unet_create": (c_int, [POINTER(UNetDesc), POINTER(c_void_p), POINTER(c_void_p), c_void_p, POINTER(c_void_p)]),
    "dt_unet_destroy": (None, [c_void_p]),
    "dt_unet_time_bias_stride": (c_int, [c_void_p]),
    "dt_unet_time_bias": (c_int, [c_void_p, c_void_p, c_void_p, c_void_p, c_int, c_void_p, c_void_p]),
    "dt_unet_workspace_bytes": (c_size_t, [c_void_p, c_int, c_int, c_int]),
    "dt_unet_forward": (c_int, [c_void_p, c_void_p, c_int, c_int, c_int, c_int, c_void_p, c_int, c_void_p,
                                c_void_p, c_size_t, c_void_p]),
    "dt_unet_autotune": (c_int, [c_void_p] + [c_int] * 5 + [c_void_p, c_size_t, c_void_p]),
    "dt_unet_conv_choice": (c_int, [c_void_p] + [c_int] * 7 + [POINTER(c_int)] * 5),
    "dt_unet_set_conv_choice": (c_int, [c_void_p] + [c_int] * 12),
    "dt_unet_set_precision": (c_int, [c_void_p, c_int]),
    "dt_unet_set_head_fusion": (c_int, [c_void_p, c_int]),
    "dt_unet_set_fused": (c_int, [c_void_p, c_int]),
    "dt_unet_fused_active": (c_int, [c_void_p, c_int, c_int]),
    "dt_unet_time_conv": (c_int, [c_void_p] + [c_int] * 13 + [c_void_p, c_size_t, c_void_p, POINTER(c_float), POINTER(c_double)]),
    "dt_unet_debug_activation": (c_int, [c_void_p, c_int, c_int, c_int, c_int, POINTER(c_size_t), POINTER(c_int),
                                         POINTER(c_int), POINTER(c_int)]),
    "dt_cfg_update": (c_int, [c_int, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, POINTER(c_float), c_int,
                              c_void_p, c_float, c_void_p, c_int, c_int, c_void_p]),
    "dt_sample_trajectory": (c_int, [c_void_p, c_int, c_int, c_int, c_int, c_int, c_int, c_void_p, POINTER(c_float),
                                     POINTER(c_int32), c_void_p, c_void_p, POINTER(c_int64), c_void_p, c_float,
                                     c_void_p, c_void_p, c_size_t, c_void_p]),
    "dt_unet_forward_mixed": (c_int, [c_void_p, c_void_p, c_int, c_int, c_int, c_int, c_void_p, c_int, c_void_p,
                                      c_void_p, c_size_t, c_void_p]),
    "dt_sample_trajectory_mixed": (c_int, [c_void_p, c_int, c_int, c_int, c_int, c_int, c_int, c_void_p, c_int,
                                           POINTER(c_float), POINTER(c_int32), c_void_p, c_void_p, POINTER(c_int64),
                                           c_void_p, c_void_p, c_void_p, c_size_t, c_void_p]),
    "dt_traj_metrics": (c_int, [c_void_p, c_void_p, c_int, c_int, c_int, c_int, c_void_p, c_void_p]),
    "dt_traj_wasserstein": (c_int, [c_void_p, c_void_p, c_int, c_int, c_int, c_void_p, c_void_p, c_int, c_void_p,
                                    c_void_p]),
    "dt_traj_pair_metrics": (c_int, [c_void_p, c_void_p, c_int, c_int, c_int, c_void_p, c_void_p, c_void_p]),
    "dt_traj_resampled_distance": (c_int, [c_void_p, c_void_p, c_int, c_int, c_int, c_int, c_void_p, c_void_p]),
    "dt_resize_bilinear": (c_int, [c_void_p, c_void_p, c_int, c_int, c_int, c_int, c_int, c_void_p]),
    "dt_pair_stats": (c_int, [c_void_p, c_void_p, c_int, c_int, c_int, c_void_p, c_void_p]),
    "dt_traj_sample_mean": (c_int, [c_void_p, c_int, c_int, c_int, c_void_p, c_void_p]),
    "dt_profile_marker": (c_int, [c_int, c_void_p]),
    "dt_profile_begin": (c_int, []),
    "dt_profile_end": (c_int, []),
    "dt_profile_class_count": (c_int, []),
    "dt_profile_read": (c_int, [c_int, POINTER(c_char_p), POINTER(c_longlong), POINTER(c_double), POINTER(c_double),
                                POINTER(c_double)]),
}

# name -> (restype, argtypes) of every symbol include/dt_hip_noise.h declares (the noise-prediction analysis, ABI 5)
NOISE_SIGNATURES = {
    "dt_q_sample": (c_int, [c_void_p, c_void_p, c_void_p, c_int, c_int, c_int, c_void_p, c_void_p]),
}

# name -> (restype, argtypes) of every symbol include/dt_hip_inception.h declares (the FID feature extractor)
INCEPTION_SIGNATURES = {
    "dt_inception_conv_desc": (c_int, [c_int, POINTER(c_int)]),
    "dt_inception_module_shape": (c_int, [c_int, POINTER(c_int), POINTER(c_int)]),
    "dt_inception_create": (c_int, [POINTER(c_void_p), c_int, c_void_p, POINTER(c_void_p)]),
    "dt_inception_destroy": (None, [c_void_p]),
    "dt_inception_workspace_bytes": (c_size_t, [c_void_p, c_int]),
    "dt_inception_preprocess": (c_int, [c_void_p, c_int, c_int, c_int, c_int, c_float, c_float, c_void_p, c_void_p]),
    "dt_inception_features": (c_int, [c_void_p, c_void_p, c_int, c_int, c_int, c_int, c_float, c_float, c_void_p,
                                      c_void_p, c_size_t, c_void_p]),
    "dt_inception_run_modules": (c_int, [c_void_p, c_int, c_int, c_void_p, c_int, c_void_p, c_void_p, c_size_t,
                                         c_void_p]),
}


# name -> (restype, argtypes) of every symbol include/dt_hip_pca.h declares (the dimensionality analysis)
PCA_SIGNATURES = {
    "dt_pca_workspace_bytes": (c_size_t, [c_int, c_int, c_int, c_int]),
    "dt_pca_fit": (c_int, [c_void_p, c_int, c_longlong, c_longlong, c_void_p, c_int, c_longlong, c_longlong, c_int, c_int,
                           c_int, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_size_t,
                           c_void_p, c_void_p]),
    "dt_pca_project": (c_int, [c_void_p, c_int, c_longlong, c_longlong, c_void_p, c_int, c_longlong, c_longlong, c_int,
                               c_int, c_int, c_void_p, c_longlong, c_void_p, c_longlong, c_void_p, c_void_p]),
}


# name -> (restype, argtypes) of every symbol include/dt_hip_fid.h declares (the Fréchet distance of the FID stage)
FID_SIGNATURES = {
    "dt_fid_workspace_bytes": (c_size_t, [c_int, c_int, c_int, c_int]),
    "dt_fid_distance": (c_int, [c_void_p, c_int, c_longlong, c_longlong, c_void_p, c_int, c_longlong, c_longlong, c_int,
                                c_int, c_void_p, c_void_p, c_void_p, c_void_p, c_size_t, c_void_p, c_void_p]),
}

# name -> (restype, argtypes) of every symbol include/dt_hip_fid_cov.h declares (the same distance by the feature-space route)
FID_COV_SIGNATURES = {
    "dt_fid_cov_workspace_bytes": (c_size_t, [c_int, c_int, c_int, c_int]),
    "dt_fid_cov_distance": FID_SIGNATURES["dt_fid_distance"],
}

# name -> (restype, argtypes) of every symbol include/dt_hip_lpips.h declares (the perceptual distance)
LPIPS_SIGNATURES = {
    "dt_lpips_create": (c_int, [POINTER(c_void_p), c_int, c_void_p, POINTER(c_void_p)]),
    "dt_lpips_destroy": (None, [c_void_p]),
    "dt_lpips_layer_shape": (c_int, [c_int, c_int, c_int, POINTER(c_int)]),
    "dt_lpips_feature_floats": (c_size_t, [c_int, c_int]),
    "dt_lpips_workspace_bytes": (c_size_t, [c_void_p, c_int, c_int, c_int]),
    "dt_lpips_features": (c_int, [c_void_p, c_void_p, c_int, c_int, c_int, c_int, c_float, c_float, c_void_p, c_void_p,
                                  c_size_t, c_void_p]),
    "dt_lpips_run_layers": (c_int, [c_void_p, c_int, c_int, c_void_p, c_int, c_int, c_int, c_void_p, c_void_p, c_size_t,
                                    c_void_p]),
    "dt_lpips_distance": (c_int, [c_void_p, c_void_p, c_int, c_void_p, c_int, c_int, c_int, c_void_p, c_void_p, c_void_p]),
    "dt_lpips_distance_many": (c_int, [c_void_p, c_void_p, c_void_p, c_int, c_int, c_int, c_int, c_void_p, c_void_p,
                                       c_void_p]),
}

# name -> (restype, argtypes) of every symbol include/dt_hip_tsne.h declares (the t-SNE of the dimensionality analysis)
TSNE_SIGNATURES = {
    "dt_tsne_workspace_bytes": (c_size_t, [c_int, c_int, c_int]),
    "dt_tsne_affinities": (c_int, [c_void_p, c_int, c_longlong, c_longlong, c_void_p, c_int, c_longlong, c_longlong, c_int,
                                   c_int, c_double, c_void_p, c_void_p, c_void_p, c_size_t, c_void_p]),
    "dt_tsne_descend": (c_int, [c_void_p, c_int, c_int, c_void_p, c_int, c_int, c_void_p, c_void_p, c_void_p, c_void_p]),
}

# name -> (restype, argtypes) of every symbol include/dt_hip_quality.h declares (KID, precision / recall, density / coverage)
QUALITY_SIGNATURES = {
    "dt_quality_workspace_bytes": (c_size_t, [c_int, c_int, c_int, c_int]),
    "dt_quality_scores": (c_int, [c_void_p, c_int, c_longlong, c_longlong, c_void_p, c_int, c_longlong, c_longlong, c_int,
                                  c_int, c_int, c_void_p, c_void_p, c_int, c_int, c_void_p, c_void_p, c_void_p, c_void_p,
                                  c_void_p, c_size_t, c_void_p, c_void_p]),
}

# name -> (restype, argtypes) of every symbol include/dt_hip_quality_stream.h declares (the same scores by row panels)
QUALITY_STREAM_SIGNATURES = {
    "dt_quality_stream_workspace_bytes": (c_size_t, [c_int, c_int, c_int, c_int, c_int]),
    "dt_quality_stream_scores": (c_int, [c_void_p, c_int, c_longlong, c_longlong, c_void_p, c_int, c_longlong, c_longlong,
                                         c_int, c_int, c_int, c_int, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p,
                                         c_size_t, c_void_p, c_void_p]),
}

# name -> (restype, argtypes) of every symbol include/dt_hip_edit.h declares (the editing stage: masked loops, hole statistics)
EDIT_SIGNATURES = {
    "dt_edit_start": (c_int, [c_void_p, c_void_p, c_int, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_int,
                              c_int, c_void_p]),
    "dt_cfg_update_masked": (c_int, [c_int, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, POINTER(c_float), c_int,
                                     c_void_p, c_float, c_void_p, c_int, c_int, c_void_p, c_void_p, c_void_p, c_void_p,
                                     c_void_p]),
    "dt_sample_trajectory_masked": (c_int, [c_void_p, c_int, c_int, c_int, c_int, c_int, c_int, c_int, c_void_p, c_int,
                                            POINTER(c_float), POINTER(c_int32), c_void_p, c_void_p, POINTER(c_int64),
                                            c_void_p, c_float, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p,
                                            c_size_t, c_void_p]),
    "dt_masked_pair_stats": (c_int, [c_void_p, c_void_p, c_int, c_int, c_int, c_void_p, c_void_p, c_void_p, c_void_p,
                                     c_void_p, c_void_p]),
}

# name -> (restype, argtypes) of every symbol include/dt_hip_rng.h declares (sampler noise: the torch CPU generator's stream)
RNG_SIGNATURES = {
    "dt_rng_mt19937_words": (c_int, [c_void_p, c_void_p, c_void_p, c_int, c_longlong, c_longlong, c_void_p, c_longlong, c_void_p,
                                     c_void_p, c_void_p]),
    "dt_rng_normal_from_words": (c_int, [c_void_p, c_longlong, c_int, c_longlong, c_longlong, c_int, c_void_p, c_longlong,
                                         c_longlong, c_longlong, c_void_p]),
    "dt_rng_workspace_bytes": (c_size_t, [c_int, c_longlong, c_int]),
    "dt_rng_randn": (c_int, [c_void_p, c_void_p, c_void_p, c_int, c_longlong, c_longlong, c_longlong, c_int, c_void_p,
                             c_longlong, c_longlong, c_longlong, c_void_p, c_void_p, c_void_p, c_size_t, c_void_p]),
}

# name -> (restype, argtypes) of every symbol include/dt_hip_align.h declares (trajectory alignment: cost matrix, DTW, Frechet)
_ALIGN_ROWS = [c_void_p, c_int, c_longlong, c_longlong, c_void_p, c_int, c_longlong, c_longlong, c_int, c_int]
ALIGN_SIGNATURES = {
    "dt_align_workspace_bytes": (c_size_t, [c_int, c_int, c_int, c_int, c_int]),
    "dt_align_min_workspace_bytes": (c_size_t, [c_int, c_int, c_int, c_int]),
    "dt_align_cost": (c_int, _ALIGN_ROWS + [c_void_p, c_void_p, c_void_p]),
    "dt_align_dp": (c_int, [c_void_p, c_int, c_int, c_int, c_int, c_int, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p,
                            c_size_t, c_void_p]),
    "dt_align": (c_int, _ALIGN_ROWS + [c_int, c_int] + [c_void_p] * 9 + [c_size_t, c_void_p]),
}

# name -> (restype, argtypes) of every symbol include/dt_hip_cka.h declares (layer-wise CKA: centred Grams, the two estimators)
_CKA_LAYERS = [POINTER(c_void_p), POINTER(c_longlong), POINTER(c_int), POINTER(c_int), POINTER(c_int), c_int]
_CKA_GRAMS = [c_void_p, c_void_p, c_void_p]
CKA_SIGNATURES = {
    "dt_cka_workspace_bytes": (c_size_t, [c_int, c_int, c_int]),
    "dt_cka_min_workspace_bytes": (c_size_t, [c_int, c_int]),
    "dt_cka_gram": (c_int, _CKA_LAYERS + [c_int] + _CKA_GRAMS + [c_void_p, c_size_t, c_void_p]),
    "dt_cka_scores": (c_int, _CKA_GRAMS + [c_int] + _CKA_GRAMS + [c_int, c_int, c_void_p, c_void_p, c_void_p, c_void_p]),
    "dt_cka": (c_int, (_CKA_LAYERS + _CKA_GRAMS) * 2 + [c_int, c_void_p, c_void_p, c_void_p, c_void_p, c_size_t, c_void_p]),
}

# name -> (restype, argtypes) of every symbol include/dt_hip_spectral.h declares (spatial-frequency spectra of the states)
_SPECTRAL_ROWS = [c_void_p, c_longlong, c_longlong]
_SPECTRAL_TAIL = [c_int] * 5 + [c_void_p, c_int, c_void_p, c_void_p, c_void_p, c_size_t, c_void_p]
SPECTRAL_SIGNATURES = {
    "dt_spectral_workspace_bytes": (c_size_t, [c_int, c_int, c_int]),
    "dt_spectral_power": (c_int, _SPECTRAL_ROWS + _SPECTRAL_TAIL),
    "dt_spectral_pair": (c_int, _SPECTRAL_ROWS * 2 + _SPECTRAL_TAIL),
    "dt_spectral_sum": (c_int, [c_void_p, c_void_p] + [c_int] * 5 + [c_void_p, c_void_p, c_void_p]),
}

# name -> (restype, argtypes) of every symbol include/dt_hip_swd.h declares (sliced Wasserstein distance between state sets)
_SWD_ROWS = [c_void_p, c_longlong, c_longlong, c_int]
_SWD_THETA = [c_void_p, c_longlong, c_int, c_int]
_SWD_SORTED = [c_void_p, c_longlong, c_void_p, c_int]
_SWD_OUT = [c_void_p] * 5 + [c_void_p, c_size_t, c_void_p]
SWD_SIGNATURES = {
    "dt_swd_sorted_bytes": (c_size_t, [c_int, c_int, c_int]),
    "dt_swd_workspace_bytes": (c_size_t, [c_int, c_int, c_int, c_int]),
    "dt_swd_distance_workspace_bytes": (c_size_t, [c_int, c_int]),
    "dt_swd_sorted": (c_int, _SWD_ROWS + [c_int] + _SWD_THETA + [c_void_p, c_void_p, c_void_p, c_size_t, c_void_p]),
    "dt_swd_distance": (c_int, _SWD_SORTED * 2 + [c_int, c_int, c_int] + _SWD_OUT),
    "dt_swd": (c_int, _SWD_ROWS * 2 + [c_int] + _SWD_THETA + [c_int] + _SWD_OUT),
}

# name -> (restype, argtypes) of every symbol include/dt_hip_sinkhorn.h declares (entropic transport cost between state sets)
_SINKHORN_SETS = _SWD_ROWS * 2 + [c_int, c_int, c_int]            # a, b, E, P, p
_SINKHORN_WS = [c_void_p, c_size_t, c_void_p]
SINKHORN_SIGNATURES = {
    "dt_sinkhorn_workspace_bytes": (c_size_t, [c_int, c_int, c_int]),
    "dt_sinkhorn_mean_cost": (c_int, _SINKHORN_SETS + [c_void_p, c_void_p] + _SINKHORN_WS),
    "dt_sinkhorn_ot": (c_int, _SINKHORN_SETS + [c_void_p, c_int, c_double] + [c_void_p] * 6 + _SINKHORN_WS),
}


class TsneParams(ctypes.Structure):
    """dt_tsne_params of include/dt_hip_tsne.h"""
    _fields_ = [("early_exaggeration", c_double), ("learning_rate", c_double), ("momentum", c_double * 2),
                ("min_gain", c_double), ("min_grad_norm", c_double), ("exaggeration_iters", c_int),
                ("n_iter_check", c_int), ("n_iter_without_progress", c_int * 2)]


def load(path=None):
    """Load (once) and return the library with argtypes set.  Raises HipLibraryError if absent."""
    global _LIB
    if _LIB is not None:
        return _LIB
    path = path or LIB_PATH
    if not os.path.exists(path):
        raise HipLibraryError(
            f"{path} is missing: the HIP extension has not been built (run "
            "`python -m distillation_trajectories_amd.csrc.build`). There is no CPU fallback.")
    import torch  # noqa: F401  -- first, so libamdhip64.so.7 resolves to the runtime torch already loaded
    try:
        lib = ctypes.CDLL(path)
    except OSError as e:
        raise HipLibraryError(f"cannot load {path}: {e}. There is no CPU fallback.") from e
    for name, (res, args) in {**SIGNATURES, **NOISE_SIGNATURES, **INCEPTION_SIGNATURES, **PCA_SIGNATURES,
                              **FID_SIGNATURES, **FID_COV_SIGNATURES, **LPIPS_SIGNATURES, **TSNE_SIGNATURES, **QUALITY_SIGNATURES,
                              **QUALITY_STREAM_SIGNATURES, **EDIT_SIGNATURES, **RNG_SIGNATURES, **ALIGN_SIGNATURES,
                              **CKA_SIGNATURES, **SPECTRAL_SIGNATURES, **SWD_SIGNATURES,
                              **SINKHORN_SIGNATURES}.items():
        try:
            fn = getattr(lib, name)
        except AttributeError as e:
            raise HipLibraryError(f"{path} does not export {name}") from e
        fn.restype, fn.argtypes = res, args
    if lib.dt_abi_version() != ABI_VERSION:
        raise HipLibraryError(f"ABI mismatch: library {lib.dt_abi_version()} vs binding {ABI_VERSION}")
    _LIB = lib
    return lib


def check(status, what):
    if status != 0:
        msg = load().dt_status_string(status)
        raise HipLibraryError(f"{what} failed with status {status}: {msg.decode() if msg else '?'}")


def ptr(t):
    """device (or host) address of a torch tensor, None -> NULL"""
    return None if t is None else c_void_p(t.data_ptr())


def stream_ptr():
    import torch
    return c_void_p(torch.cuda.current_stream().cuda_stream)


class DeviceHandle:
    """A library handle on one device: the tensors moved there and given to ``<ENTRY>_create`` as a pointer array,
    ``<ENTRY>_destroy`` when the object goes, and a workspace of ``<ENTRY>_workspace_bytes`` grown on demand."""
    ENTRY = None            # the entry points' prefix, "dt_inception"
    GPU_ONLY = None         # what runs on the GPU only, for the error message

    def __init__(self, tensors, device):
        import torch
        self.device = torch.device(device)
        if self.device.type != "cuda":
            raise HipLibraryError(f"{self.GPU_ONLY} on the GPU only, got device {self.device}")
        with torch.cuda.device(self.device):
            dev = [t.detach().to(self.device, torch.float32).contiguous() for t in tensors]
            arr = (c_void_p * len(dev))(*[t.data_ptr() for t in dev])
            h = c_void_p()
            create = f"{self.ENTRY}_create"
            check(getattr(load(), create)(arr, len(dev), stream_ptr(), ctypes.byref(h)), create)
        self._h = h
        self._ws = None

    def __del__(self):
        h = getattr(self, "_h", None)
        if h is not None and h.value:
            getattr(load(), f"{self.ENTRY}_destroy")(h)
            self._h = None

    def workspace(self, *shape):
        """The workspace for a batch of ``shape`` (the arguments of ``<ENTRY>_workspace_bytes`` after the handle)."""
        import torch
        need = getattr(load(), f"{self.ENTRY}_workspace_bytes")(self._h, *shape)
        if self._ws is None or self._ws.numel() < need:
            self._ws = torch.empty(need, dtype=torch.uint8, device=self.device)
        return self._ws


def profile_marker(marker_id):
    """Empty, recognisably named kernel on the current stream (brackets a region for external profilers)."""
    check(load().dt_profile_marker(int(marker_id), stream_ptr()), "dt_profile_marker")


def profile_begin():
    check(load().dt_profile_begin(), "dt_profile_begin")


def profile_end():
    """Stop recording and return {kernel class: dict(launches, ms, flops, bytes)} (stream must be synchronised)."""
    lib = load()
    check(lib.dt_profile_end(), "dt_profile_end")
    out = {}
    for cls in range(lib.dt_profile_class_count()):
        name, n, ms, fl, by = c_char_p(), c_longlong(), c_double(), c_double(), c_double()
        check(lib.dt_profile_read(cls, ctypes.byref(name), ctypes.byref(n), ctypes.byref(ms), ctypes.byref(fl),
                                  ctypes.byref(by)), "dt_profile_read")
        if n.value:
            out[name.value.decode()] = dict(launches=n.value, ms=ms.value, flops=fl.value, bytes=by.value)
    return out
