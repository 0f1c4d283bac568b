"""Build libdt_hip.so in-tree with hipcc for gfx950 (no torch headers, pure HIP runtime + C ABI).

``python -m distillation_trajectories_amd.csrc.build`` or ``build()`` from ``__graft_entry__``.
The library is linked against ``libamdhip64.so.7`` by SONAME only (no rpath), so inside a Python
process that has already imported torch it binds to the HIP runtime torch itself loaded and shares
its streams and allocations.
"""
import os
import shutil
import subprocess
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
SOURCES = ["dt_conv.hip", "dt_conv_bf16.hip", "dt_conv_strip.hip", "dt_conv_strip_pair.hip", "dt_layers.hip", "dt_update.hip", "dt_metrics.hip", "dt_fused.hip", "dt_profile.hip", "dt_unet.hip",
           "dt_unet_forward.hip", "dt_unet_tune.hip", "dt_sample.hip", "dt_featnet.hip", "dt_inception.hip", "dt_pca.hip", "dt_fid.hip", "dt_lpips.hip", "dt_tsne.hip", "dt_quality.hip", "dt_quality_stream.hip", "dt_edit.hip", "dt_rng.hip", "dt_align.hip", "dt_cka.hip", "dt_spectral.hip", "dt_swd.hip", "dt_sinkhorn.hip"]
HEADERS = ["dt_internal.h", "dt_conv_forms.h", "dt_conv_rows.h", "dt_batch.h", "dt_dense64.h", "dt_quality_math.h", "dt_featnet.h", "dt_conv_epilogue.h", "dt_conv_walk.h", "dt_conv_strip_kernel.h", "dt_conv_strip_pair.h", "dt_update_math.h", "dt_fused.h", "dt_unet.h", "dt_unet_layout.h", os.path.join("..", "..", "include", "dt_hip.h"),
           os.path.join("..", "..", "include", "dt_hip_noise.h"),
           os.path.join("..", "..", "include", "dt_hip_inception.h"),
           os.path.join("..", "..", "include", "dt_hip_pca.h"),
           os.path.join("..", "..", "include", "dt_hip_fid.h"),
           os.path.join("..", "..", "include", "dt_hip_fid_cov.h"),
           os.path.join("..", "..", "include", "dt_hip_lpips.h"),
           os.path.join("..", "..", "include", "dt_hip_tsne.h"),
           os.path.join("..", "..", "include", "dt_hip_quality.h"),
           os.path.join("..", "..", "include", "dt_hip_quality_stream.h"),
           os.path.join("..", "..", "include", "dt_hip_edit.h"),
           os.path.join("..", "..", "include", "dt_hip_rng.h"),
           os.path.join("..", "..", "include", "dt_hip_align.h"),
           os.path.join("..", "..", "include", "dt_hip_cka.h"),
           os.path.join("..", "..", "include", "dt_hip_spectral.h"),
           os.path.join("..", "..", "include", "dt_hip_swd.h"),
           os.path.join("..", "..", "include", "dt_hip_sinkhorn.h")]
LIB = os.path.join(HERE, "libdt_hip.so")
ARCH = "gfx950"


def hipcc_path():
    for cand in (os.environ.get("HIPCC"), "/opt/rocm/bin/hipcc", shutil.which("hipcc")):
        if cand and os.path.exists(cand):
            return cand
    raise RuntimeError("hipcc not found (looked at $HIPCC, /opt/rocm/bin/hipcc, PATH)")


OBJ_DIR = os.path.join(HERE, "_build")
# no -fgpu-flush-denormals-to-zero here: dt_rng.hip is bit-equal to torch.randn only with fp32 denormals kept (the default)
FLAGS = [f"--offload-arch={ARCH}", "-O3", "-std=c++17", "-fPIC", "-Wall", "-Wno-unused-function"]


def _newer(target, deps):
    if not os.path.exists(target):
        return True
    t = os.path.getmtime(target)
    return any(os.path.getmtime(d) > t for d in deps)


def is_stale():
    deps = [os.path.join(HERE, f) for f in SOURCES + HEADERS] + [os.path.abspath(__file__)]
    return _newer(LIB, deps)


def build(force=False, verbose=False):
    """Compile every HIP source for gfx950 (one object per source, in parallel, only what changed unless
    ``force``) and link the shared library.  Returns its path."""
    if not force and not is_stale():
        return LIB
    from concurrent.futures import ThreadPoolExecutor
    os.makedirs(OBJ_DIR, exist_ok=True)
    hipcc = hipcc_path()
    common = [os.path.join(HERE, f) for f in HEADERS] + [os.path.abspath(__file__)]

    def compile_one(src):
        obj = os.path.join(OBJ_DIR, src.replace(".hip", ".o"))
        path = os.path.join(HERE, src)
        if not force and not _newer(obj, [path] + common):
            return obj, None
        cmd = [hipcc] + FLAGS + ["-c", path, "-o", obj]
        if verbose:
            print(" ".join(cmd), flush=True)
        return obj, subprocess.run(cmd, capture_output=True, text=True)

    # (at most 16: a shared machine may show many more CPUs than the build is allotted)
    with ThreadPoolExecutor(max_workers=min(len(SOURCES), os.cpu_count() or 1, 16)) as pool:
        results = list(pool.map(compile_one, SOURCES))
    for obj, res in results:
        if res is None:
            continue
        if res.returncode != 0:
            sys.stderr.write(res.stdout + res.stderr)
            raise RuntimeError(f"hipcc failed with exit code {res.returncode} on {obj}")
        if verbose and res.stderr:
            sys.stderr.write(res.stderr)
    cmd = [hipcc, f"--offload-arch={ARCH}", "-shared", "-fPIC", "-fno-rtlib-add-rpath", "-o", LIB] + [o for o, _ in results]
    if verbose:
        print(" ".join(cmd), flush=True)
    res = subprocess.run(cmd, capture_output=True, text=True)
    if res.returncode != 0:
        sys.stderr.write(res.stdout + res.stderr)
        raise RuntimeError(f"hipcc link failed with exit code {res.returncode}")
    return LIB


SAN_DRIVER = os.path.join(OBJ_DIR, "dt_host_sanitize")


NOISE_SAN_DRIVER = os.path.join(OBJ_DIR, "dt_host_sanitize_noise")
INCEPTION_SAN_DRIVER = os.path.join(OBJ_DIR, "dt_host_sanitize_inception")
PCA_SAN_DRIVER = os.path.join(OBJ_DIR, "dt_host_sanitize_pca")
FID_SAN_DRIVER = os.path.join(OBJ_DIR, "dt_host_sanitize_fid")
LPIPS_SAN_DRIVER = os.path.join(OBJ_DIR, "dt_host_sanitize_lpips")
ALIGN_SAN_DRIVER = os.path.join(OBJ_DIR, "dt_host_sanitize_align")
CKA_SAN_DRIVER = os.path.join(OBJ_DIR, "dt_host_sanitize_cka")
SPECTRAL_SAN_DRIVER = os.path.join(OBJ_DIR, "dt_host_sanitize_spectral")
SWD_SAN_DRIVER = os.path.join(OBJ_DIR, "dt_host_sanitize_swd")
SINKHORN_SAN_DRIVER = os.path.join(OBJ_DIR, "dt_host_sanitize_sinkhorn")


def build_sanitizer_driver(verbose=False, driver="driver.cpp", out=SAN_DRIVER, sources=None):
    """tests/host_sanitize/<driver> + every library source, HOST code instrumented with AddressSanitizer and
    UndefinedBehaviorSanitizer (``-Xarch_host -fsanitize=...``; device code is left alone: GPU ASan is unavailable on this
    pool), one executable (default csrc/_build/dt_host_sanitize).  Cross-compiles without a GPU; tests/test_host_sanitize.py
    runs it on the GPU box."""
    hipcc = hipcc_path()
    os.makedirs(OBJ_DIR, exist_ok=True)
    root = os.path.dirname(os.path.dirname(HERE))
    driver = os.path.join(root, "tests", "host_sanitize", driver)
    sources = SOURCES if sources is None else sources
    deps = [os.path.join(HERE, f) for f in sources + HEADERS] + [driver, os.path.abspath(__file__)]
    if not _newer(out, deps):
        return out
    san = ["-Xarch_host", "-fsanitize=address", "-Xarch_host", "-fsanitize=undefined", "-Xarch_host", "-fno-omit-frame-pointer"]
    cmd = ([hipcc, f"--offload-arch={ARCH}", "-O1", "-g", "-std=c++17", "-Wno-unused-function", "-x", "hip"] + san +
           [os.path.join(HERE, f) for f in sources] + [driver, "-o", out])
    if verbose:
        print(" ".join(cmd), flush=True)
    res = subprocess.run(cmd, capture_output=True, text=True)
    if res.returncode != 0:
        sys.stderr.write(res.stdout + res.stderr)
        raise RuntimeError(f"sanitizer driver build failed with exit code {res.returncode}")
    return out


def build_noise_sanitizer_driver(verbose=False):
    """The same instrumented build around tests/host_sanitize/noise_driver.cpp, which walks every entry point of
    include/dt_hip_noise.h: csrc/_build/dt_host_sanitize_noise (run by tests/test_hip_noise_analysis.py)."""
    return build_sanitizer_driver(verbose, driver="noise_driver.cpp", out=NOISE_SAN_DRIVER)


def build_inception_sanitizer_driver(verbose=False):
    """The same instrumented build around tests/host_sanitize/inception_driver.cpp, which walks every entry point of
    include/dt_hip_inception.h: csrc/_build/dt_host_sanitize_inception (run by tests/test_hip_inception.py)."""
    return build_sanitizer_driver(verbose, driver="inception_driver.cpp", out=INCEPTION_SAN_DRIVER)


def build_pca_sanitizer_driver(verbose=False):
    """The same instrumented build around tests/host_sanitize/pca_driver.cpp, which walks every entry point of
    include/dt_hip_pca.h: csrc/_build/dt_host_sanitize_pca (run by tests/test_hip_pca.py)."""
    return build_sanitizer_driver(verbose, driver="pca_driver.cpp", out=PCA_SAN_DRIVER)


def build_fid_sanitizer_driver(verbose=False):
    """The same instrumented build around tests/host_sanitize/fid_driver.cpp, which walks every entry point of
    include/dt_hip_fid.h: csrc/_build/dt_host_sanitize_fid (run by tests/test_hip_fid.py)."""
    return build_sanitizer_driver(verbose, driver="fid_driver.cpp", out=FID_SAN_DRIVER)


def build_lpips_sanitizer_driver(verbose=False):
    """The same instrumented build around tests/host_sanitize/lpips_driver.cpp, which walks every entry point of
    include/dt_hip_lpips.h: csrc/_build/dt_host_sanitize_lpips (run by tests/test_hip_lpips.py)."""
    return build_sanitizer_driver(verbose, driver="lpips_driver.cpp", out=LPIPS_SAN_DRIVER)


def build_align_sanitizer_driver(verbose=False):
    """tests/host_sanitize/align_driver.cpp with csrc/dt_align.hip alone, host code instrumented in the same way: the workspace
    queries and argument errors of include/dt_hip_align.h, none of which reaches the GPU: csrc/_build/dt_host_sanitize_align
    (run by tests/test_align_host.py, without a GPU)."""
    return build_sanitizer_driver(verbose, driver="align_driver.cpp", out=ALIGN_SAN_DRIVER, sources=["dt_align.hip"])


def build_cka_sanitizer_driver(verbose=False):
    """tests/host_sanitize/cka_driver.cpp with csrc/dt_cka.hip alone, host code instrumented in the same way: the workspace
    arithmetic and argument errors of include/dt_hip_cka.h, none of which reaches the GPU: csrc/_build/dt_host_sanitize_cka
    (run by tests/test_cka_host.py, without a GPU)."""
    return build_sanitizer_driver(verbose, driver="cka_driver.cpp", out=CKA_SAN_DRIVER, sources=["dt_cka.hip"])


def build_spectral_sanitizer_driver(verbose=False):
    """tests/host_sanitize/spectral_driver.cpp with csrc/dt_spectral.hip (and csrc/dt_profile.hip, whose ProfileScope it opens),
    host code instrumented in the same way: the workspace query and argument errors of include/dt_hip_spectral.h, none of
    which reaches the GPU: csrc/_build/dt_host_sanitize_spectral (run by tests/test_spectral_host.py, without a GPU)."""
    return build_sanitizer_driver(verbose, driver="spectral_driver.cpp", out=SPECTRAL_SAN_DRIVER,
                                  sources=["dt_spectral.hip", "dt_profile.hip"])


def build_swd_sanitizer_driver(verbose=False):
    """tests/host_sanitize/swd_driver.cpp with csrc/dt_swd.hip (and csrc/dt_profile.hip, whose ProfileScope it opens), host
    code instrumented in the same way: the size queries and argument errors of include/dt_hip_swd.h, none of which reaches
    the GPU: csrc/_build/dt_host_sanitize_swd (run by tests/test_swd_host.py, without a GPU)."""
    return build_sanitizer_driver(verbose, driver="swd_driver.cpp", out=SWD_SAN_DRIVER, sources=["dt_swd.hip", "dt_profile.hip"])


def build_sinkhorn_sanitizer_driver(verbose=False):
    """tests/host_sanitize/sinkhorn_driver.cpp with csrc/dt_sinkhorn.hip (and csrc/dt_profile.hip, whose ProfileScope it opens),
    host code instrumented in the same way: the size query and argument errors of include/dt_hip_sinkhorn.h, none of which
    reaches the GPU: csrc/_build/dt_host_sanitize_sinkhorn (run by tests/test_sinkhorn_host.py, without a GPU)."""
    return build_sanitizer_driver(verbose, driver="sinkhorn_driver.cpp", out=SINKHORN_SAN_DRIVER,
                                  sources=["dt_sinkhorn.hip", "dt_profile.hip"])


if __name__ == "__main__":
    print(build(force="--force" in sys.argv, verbose=True))
    if "--sanitize" in sys.argv:
        print(build_sanitizer_driver(verbose=True))
        print(build_noise_sanitizer_driver(verbose=True))
        print(build_inception_sanitizer_driver(verbose=True))
        print(build_pca_sanitizer_driver(verbose=True))
        print(build_fid_sanitizer_driver(verbose=True))
        print(build_lpips_sanitizer_driver(verbose=True))
        print(build_align_sanitizer_driver(verbose=True))
        print(build_cka_sanitizer_driver(verbose=True))
        print(build_spectral_sanitizer_driver(verbose=True))
        print(build_swd_sanitizer_driver(verbose=True))
        print(build_sinkhorn_sanitizer_driver(verbose=True))
