"""GPU: LPIPS v0.1, net='alex' (include/dt_hip_lpips.h, csrc/dt_lpips.hip) against the float64 restatement
(tests/lpips_ref64.py) on random weights: every layer on the device's own upstream output, the whole network, the distance
on independent and on near pairs, the exact properties of the distance kernel, argument errors, compute_lpips and
lpips_sweep."""
import os
import subprocess

import numpy as np
import pytest
import torch

import lpips_ref64 as ref
from distillation_trajectories_amd import _hip, lpips
from distillation_trajectories_amd.evaluation.metrics import LPIPSModel, compute_lpips, lpips_distances

DEV = torch.device("cuda:0")
pytestmark = pytest.mark.gpu

# Per-image relative L2 error against float64.
# One layer fed the device's own upstream output: the bound of the Inception modules (tests/test_hip_inception.py
# MODULE_TOL), the same arithmetic -- a k-ordered fp32 MFMA chain, K at most 3456 here against Inception's 3 * 3 * 448 = 4032.
LAYER_TOL = 2e-6
# Tap l of the whole network: layers 0..l each add at most LAYER_TOL of their own, and what a layer inherits passes through a
# He-scaled conv + ReLU (gain about 1 on a random perturbation) and, for two layers, a max pool that keeps one of nine values;
# a factor 2 covers those: 2 * (l + 1) * LAYER_TOL.
NETWORK_TOL = [2 * (l + 1) * LAYER_TOL for l in range(5)]

# The distance.  The yardstick is the fp32 torch-CPU evaluation of the same restatement on the same inputs -- what the lpips
# package itself computes -- against float64: its maximum relative errors (total, per layer) as tests/test_lpips_host.py
# measures and records them.  The device must stay within 4 x: MFMA's k order and the CPU library's blocked order are two
# fp32 summation orders of the same sums.  Measured device maxima: DESIGN.md section 9.
YARDSTICK = {"independent": (1.78e-7, 1.04e-6), "near": (2.59e-6, 1.14e-5)}
DISTANCE_BOUND = {k: (4 * t, 4 * p) for k, (t, p) in YARDSTICK.items()}

SIZES = list(ref.SIZES)


@pytest.fixture(scope="module")
def weights():
    """(float64 state dict, float32 state dict): the float64 one is the float32 one widened, the same network"""
    sd32 = ref.random_state_dict(11, torch.float32)
    return ref.cast(sd32, torch.float64), sd32


@pytest.fixture(scope="module")
def model(weights):
    return LPIPSModel(DEV, weights=weights[1])


def _rel_per_image(got, want):
    got, want = got.double().cpu().flatten(1), want.double().cpu().flatten(1)
    return ((got - want).norm(dim=1) / want.norm(dim=1)).numpy()


def test_lpips_entry_host_code_clean_under_asan_and_ubsan():
    """tests/host_sanitize/lpips_driver.cpp (every entry of include/dt_hip_lpips.h) under host ASan / UBSan."""
    from distillation_trajectories_amd.csrc.build import LPIPS_SAN_DRIVER, build_lpips_sanitizer_driver
    if not os.path.exists(LPIPS_SAN_DRIVER):
        build_lpips_sanitizer_driver()
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=0:halt_on_error=1:abort_on_error=0",
               UBSAN_OPTIONS="print_stacktrace=1:halt_on_error=1")
    r = subprocess.run([LPIPS_SAN_DRIVER], capture_output=True, text=True, env=env, timeout=300)
    report = r.stdout[-3000:] + "\n" + r.stderr[-6000:]
    assert "AddressSanitizer" not in r.stderr and "runtime error:" not in r.stderr, report
    assert r.returncode == 0 and "lpips driver ok" in r.stdout, report


@pytest.mark.parametrize("hw", SIZES)
def test_every_layer_on_its_own_upstream_output(weights, model, hw):
    """Each layer through the layer-range entry, fed the device's own output of the layer before (the fp32 scaled image for
    layer 0), against float64 on that same input."""
    sd = weights[0]
    H, W = hw
    x = ref.scale_input(weights[1], ref.images(5, H, W, seed=21 + H)).permute(0, 2, 3, 1).contiguous().to(DEV)
    worst = []
    for l in range(lpips.N_LAYERS):
        y = model.handle.run_layers(x, l, l + 1, H, W)
        want = ref.run_layer(sd, l, x.double().cpu().permute(0, 3, 1, 2))
        got = y.permute(0, 3, 1, 2)
        assert tuple(got.shape) == tuple(want.shape), l
        rel = _rel_per_image(got, want)
        worst.append(float(rel.max()))
        assert rel.max() <= LAYER_TOL, f"layer {l} at {hw}: per-image relative L2 {rel.max():.3g}"
        x = y
    print(f"layer maxima {hw}", [f"{v:.2e}" for v in worst])
    # the whole range in one call is the chain of single layers
    x0 = ref.scale_input(weights[1], ref.images(5, H, W, seed=21 + H)).permute(0, 2, 3, 1).contiguous().to(DEV)
    assert torch.equal(model.handle.run_layers(x0, 0, lpips.N_LAYERS, H, W), x)


@pytest.mark.parametrize("hw", SIZES)
@pytest.mark.parametrize("N", [1, 37])
@pytest.mark.parametrize("in_map", [(2.0, -1.0), (1.0, 0.0)])
def test_whole_network_against_float64(weights, model, hw, N, in_map):
    H, W = hw
    imgs = ref.images(N, H, W, seed=N * 7 + W)
    if in_map[0] == 2.0:
        imgs = (imgs + 1) / 2
    pack = model.handle.features(imgs, *in_map)
    assert tuple(pack.shape) == (N, lpips.feature_floats(H, W))
    want = ref.taps(weights[0], imgs.double(), *in_map)
    for l, (got, w) in enumerate(zip(lpips.split_pack(pack, H, W), want)):
        assert tuple(got.shape[1:]) == lpips.layer_shape(H, W, l) == (w.shape[2], w.shape[3], w.shape[1])
        rel = _rel_per_image(got.permute(0, 3, 1, 2), w)
        print(f"network {hw} N={N} map={in_map} tap {l}: max per-image relative L2 {rel.max():.2e}")
        assert rel.max() <= NETWORK_TOL[l], f"tap {l} {hw} N={N} {in_map}: {rel.max():.3g}"
        assert (got != 0).double().mean().item() > 0.3, f"tap {l} is mostly dead"


@pytest.mark.parametrize("kind", ["independent", "near"])
def test_distance_against_float64(weights, model, kind):
    """Totals and layer terms against float64, within 4 x the fp32 restatement's own error for the same kind of pair."""
    worst_t = worst_l = 0.0
    for hw in SIZES:
        a, b = ref.pair_inputs(hw, kind)
        total = lpips_distances(a, b, model, in_scale=1.0, in_shift=0.0)
        layers = lpips_distances(a, b, model, in_scale=1.0, in_shift=0.0, per_layer=True)
        d64, l64 = ref.distance(weights[0], a, b)
        t, p = ref.relative_errors(total.cpu(), layers.cpu(), d64, l64)
        print(f"distance {kind} {hw}: total {t:.3g}, per layer {p:.3g}")
        worst_t, worst_l = max(worst_t, t), max(worst_l, p)
    print(f"distance {kind}: device maxima total {worst_t:.3g}, per layer {worst_l:.3g}; bounds {DISTANCE_BOUND[kind]}")
    assert worst_t <= DISTANCE_BOUND[kind][0] and worst_l <= DISTANCE_BOUND[kind][1]


def test_distance_exact_properties(model):
    H, W = 35, 47
    a, b = ref.images(37, H, W, seed=51), ref.images(37, H, W, seed=52)
    h = model.handle
    pa, pb = h.features(a), h.features(b)
    d_ab, l_ab = h.distance(pa, pb, H, W, per_layer=True)
    d_ba, l_ba = h.distance(pb, pa, H, W, per_layer=True)
    assert torch.equal(d_ab, d_ba) and torch.equal(l_ab, l_ba)                       # symmetry, bit for bit
    zero, zl = h.distance(pa, pa.clone(), H, W, per_layer=True)
    assert torch.equal(zero, torch.zeros_like(zero)) and torch.equal(zl, torch.zeros_like(zl))
    assert (d_ab > 0).all() and torch.equal(d_ab, h.distance(pa, pb, H, W))          # repeatable, with and without layers
    # one shared reference image equals the expanded call
    shared = h.distance(pa[3:4], pb, H, W)
    assert torch.equal(shared, h.distance(pa[3:4].expand(37, -1).contiguous(), pb, H, W))
    assert torch.equal(shared[3], d_ab[3])
    # a pair's bits do not depend on the batch it is in
    for bs in (1, 5, 16):
        parts = [h.distance(pa[i:i + bs], pb[i:i + bs], H, W) for i in range(0, 37, bs)]
        assert torch.equal(torch.cat(parts), d_ab), bs
    # distance_many equals G distance calls
    G = 3
    students = torch.stack([pb, pa, pb.flip(0)])
    many, many_l = h.distance_many(pa, students, H, W, per_layer=True)
    for g in range(G):
        dg, lg = h.distance(pa, students[g], H, W, per_layer=True)
        assert torch.equal(many[g], dg) and torch.equal(many_l[g], lg), g
    assert torch.equal(many[1], torch.zeros_like(many[1]))


def test_features_independent_of_batching_workspace_and_repeatable(model):
    H, W = 35, 47
    imgs = ref.images(37, H, W, seed=5)
    h = model.handle
    full = h.features(imgs)
    assert torch.equal(full, h.features(imgs))
    for bs in (1, 5, 16):
        got = torch.cat([h.features(imgs[i:i + bs]) for i in range(0, 37, bs)])
        assert torch.equal(got, full), bs
    other = torch.cat([ref.images(3, H, W, seed=6), imgs[10:11], ref.images(2, H, W, seed=7)])
    assert torch.equal(h.features(other)[3], full[10])
    # a poisoned, a larger and an offset workspace change nothing
    lib = _hip.load()
    x = imgs[:6].to(DEV).contiguous()
    want = full[:6]
    need = lib.dt_lpips_workspace_bytes(h._h, 6, H, W)
    big = torch.empty(2 * need + 4096, dtype=torch.uint8, device=DEV)
    for poison, off, size in ((float("nan"), 0, need), (1e30, 0, 2 * need), (float("nan"), 4096, need + 64)):
        big.view(torch.float32).fill_(poison)
        out = torch.empty_like(want)
        ws = big[off:off + size]
        with torch.cuda.device(DEV):
            st = lib.dt_lpips_features(h._h, _hip.ptr(x), 6, 3, H, W, 1.0, 0.0, _hip.ptr(out), _hip.ptr(ws), size,
                                       _hip.stream_ptr())
        assert st == 0 and torch.equal(out, want), (poison, off, size)


def test_argument_errors_give_a_status_and_leave_the_output_alone(model):
    lib, h = _hip.load(), model.handle
    SENT = 12345.0
    sp = _hip.stream_ptr()

    def features(N, C, H, W, ws_short=0, F=None):
        x = torch.zeros(N, C, H, W, device=DEV)
        F = F or lpips.feature_floats(32, 32)
        out = torch.full((N, F), SENT, device=DEV)
        ws = torch.empty(max(lib.dt_lpips_workspace_bytes(h._h, N, 32, 32), 64), dtype=torch.uint8, device=DEV)
        size = ws.numel() - ws_short
        if 31 <= H <= 299 and 31 <= W <= 299:
            size = lib.dt_lpips_workspace_bytes(h._h, N, H, W) - ws_short
            ws = torch.empty(size + ws_short, dtype=torch.uint8, device=DEV)
        st = lib.dt_lpips_features(h._h, _hip.ptr(x), N, C, H, W, 1.0, 0.0, _hip.ptr(out), _hip.ptr(ws), size, sp)
        torch.cuda.synchronize()
        assert torch.equal(out, torch.full_like(out, SENT))
        return st

    assert features(2, 3, 30, 30) == -2                      # DT_E_SHAPE
    assert features(2, 3, 300, 300) == -2
    assert features(2, 1, 32, 32) == -2                      # C = 1
    assert features(2, 3, 32, 32, ws_short=4) == -4          # DT_E_WORKSPACE
    # n0 = 2 with n1 = 3
    F = lpips.feature_floats(32, 32)
    p0, p1 = torch.rand(2, F, device=DEV), torch.rand(3, F, device=DEV)
    dist, layers = torch.full((3,), SENT, device=DEV), torch.full((3, 5), SENT, device=DEV)
    assert lib.dt_lpips_distance(h._h, _hip.ptr(p0), 2, _hip.ptr(p1), 3, 32, 32, _hip.ptr(dist), _hip.ptr(layers), sp) == -3
    assert lib.dt_lpips_distance(h._h, _hip.ptr(p0), 1, _hip.ptr(p1), 3, 30, 30, _hip.ptr(dist), _hip.ptr(layers), sp) == -2
    assert lib.dt_lpips_distance(h._h, _hip.ptr(p0), 1, _hip.ptr(p1), 3, 300, 300, _hip.ptr(dist), _hip.ptr(layers), sp) == -2
    torch.cuda.synchronize()
    assert torch.equal(dist, torch.full_like(dist, SENT)) and torch.equal(layers, torch.full_like(layers, SENT))
    # the Python layer raises ValueError before any call
    with pytest.raises(ValueError, match="30x30"):
        h.features(torch.zeros(1, 3, 30, 30))
    with pytest.raises(ValueError, match="300x300"):
        h.features(torch.zeros(1, 3, 300, 300))
    with pytest.raises(ValueError, match="3 channels"):
        h.features(torch.zeros(1, 1, 32, 32))
    with pytest.raises(ValueError, match="one image or as many"):
        h.distance(p0, p1, 32, 32)


def test_compute_lpips_on_one_pair_in_unit_range(weights, model):
    a, b = (ref.images(1, 64, 64, seed=71) + 1) / 2, (ref.images(1, 64, 64, seed=72) + 1) / 2
    got = compute_lpips(a, b, DEV, model=model)
    assert isinstance(got, float)
    want = ref.distance(weights[0], a.double(), b.double(), 2.0, -1.0)[0].item()
    print(f"compute_lpips {got!r} float64 {want!r} relative error {abs(got - want) / want:.3g}")
    assert abs(got - want) <= DISTANCE_BOUND["independent"][0] * want
    assert compute_lpips(a[0], b[0], DEV, weights=weights[1]) == got                     # [3, H, W], a model of its own
    assert compute_lpips(a, a, DEV, model=model) == 0.0


def test_largest_input_runs(model):
    """299 x 299, the largest size the entry takes: shapes, finite values, d(x, x) == 0 and a positive distance."""
    a, b = ref.images(2, 299, 299, seed=81), ref.images(2, 299, 299, seed=82)
    pa = model.handle.features(a)
    assert tuple(pa.shape) == (2, 74 * 74 * 64 + 36 * 36 * 192 + 17 * 17 * (384 + 256 + 256)) and torch.isfinite(pa).all()
    d = lpips_distances(a, b, model, in_scale=1.0, in_shift=0.0)
    assert (d > 0).all() and torch.equal(lpips_distances(a, a, model, 1.0, 0.0), torch.zeros(2, device=DEV))


def _models(image_size, timesteps):
    from distillation_trajectories_amd.config import Config
    from distillation_trajectories_amd.models import DiffusionUNet
    from distillation_trajectories_amd.synthetic import make_model
    cfg = Config()
    cfg.image_size, cfg.timesteps = image_size, timesteps
    return cfg, [make_model(DiffusionUNet, cfg, sf).to(DEV) for sf in (1.0, 0.2, 0.5)]


def test_lpips_sweep_equals_lpips_distances_on_the_grid_states(model):
    from distillation_trajectories_amd import engine
    from distillation_trajectories_amd.analysis.metrics.perceptual import lpips_sweep
    from distillation_trajectories_amd.analysis.trajectory_engine import sample_grid
    from distillation_trajectories_amd.synthetic import noise_table
    cfg, (teacher, s02, s05) = _models(32, 4)
    T, S, scales = 4, 3, [1.0, 3.0]
    res = lpips_sweep(teacher, [s02, s05, teacher], cfg, scales, S, model=model, every=2)
    assert res["states"] == [0, 2, 4]
    assert res["lpips"].shape == (3, 2, 3, S) and res["per_layer"].shape == (3, 2, 3, S, 5)
    assert res["lpips"].dtype == np.float32
    assert np.array_equal(res["lpips"][2], np.zeros((2, 3, S), np.float32))          # the teacher against itself
    assert np.array_equal(res["lpips"][:, :, 0], np.zeros((3, 2, S), np.float32))    # every model starts from the same noise
    assert (res["lpips"][:2, :, 1:] > 0).all()
    table = noise_table(42, S + T - 1, (1, 3, 32, 32)).reshape(S + T - 1, -1).to(DEV)
    grids = [sample_grid(engine.UNetHandle.for_module(m), table, 0, S, T, scales, 32, 32) for m in (teacher, s02, s05)]
    for i_s in (0, 1):
        for i_g, gs in enumerate(scales):
            for i_t, t in enumerate(res["states"]):
                x0 = grids[0][gs][t].reshape(S, 3, 32, 32)
                x1 = grids[1 + i_s][gs][t].reshape(S, 3, 32, 32)
                want = lpips_distances(x0, x1, model, in_scale=1.0, in_shift=0.0, per_layer=True)
                assert np.array_equal(res["per_layer"][i_s, i_g, i_t], want.cpu().numpy()), (i_s, gs, t)
                total = lpips_distances(x0, x1, model, in_scale=1.0, in_shift=0.0)
                assert np.array_equal(res["lpips"][i_s, i_g, i_t], total.cpu().numpy()), (i_s, gs, t)


def test_lpips_sweep_resizes_16_pixel_configs(model):
    from distillation_trajectories_amd.analysis.metrics.perceptual import lpips_sweep
    cfg, (teacher, s02, _) = _models(16, 3)
    with pytest.raises(ValueError, match="16x16"):
        lpips_sweep(teacher, [s02], cfg, [1.0], 2, model=model)
    res = lpips_sweep(teacher, [s02], cfg, [1.0], 2, model=model, resize=(32, 40))
    assert res["lpips"].shape == (1, 1, 4, 2) and np.isfinite(res["lpips"]).all() and (res["lpips"][0, 0, -1] > 0).all()
