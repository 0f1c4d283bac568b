"""GPU: sampler noise on the device (include/dt_hip_rng.h, csrc/dt_rng.hip, engine.device_mt19937_words / device_randn)
against the float32 yardstick tests/randn_ref.py, the recorded torch vectors and, where the host's CPU capability is the
recorded one, live ``torch.randn``.  Every comparison is of bits; there is no tolerance in this file."""
import json
import os

import numpy as np
import pytest
import torch

import randn_ref
from distillation_trajectories_amd import _hip, engine

DEV = torch.device("cuda:0")
pytestmark = pytest.mark.gpu
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
with open(os.path.join(GOLDEN, "torch_randn_vectors.json")) as _f:
    META = json.load(_f)
SEEDS = [0, 42, 2 ** 32 - 1, 2 ** 32 + 5]
ELEMENTS = [16, 20, 105, 768, 3072]


def u32(t):
    """the uint32 bits of a device int32 / float32 tensor, on the host"""
    return t.detach().cpu().contiguous().numpy().view(np.uint32)


def host_matches_golden():
    return torch.backends.cpu.get_cpu_capability() == META["cpu_capability"]


# ------------------------------------------------------------------------------------------------ words
@pytest.mark.parametrize("seed", SEEDS)
def test_words_equal_yardstick(seed):
    for n in (1, 623, 624, 625, 2000):
        for skip in (0, 1, 397, 624, 1000):
            got, (st, pos) = engine.device_mt19937_words(seeds=seed, n=n, skip=skip, device=DEV, return_state=True)
            want, end = randn_ref.mt19937_words(seed, n, skip=skip)
            assert np.array_equal(u32(got)[0], want), (seed, n, skip)
            assert int(pos[0]) == end.pos and np.array_equal(u32(st)[0], end.state), (seed, n, skip)


def test_words_continue_from_end_state():
    long_walk = u32(engine.device_mt19937_words(seeds=42, n=3000, skip=5, device=DEV))[0]
    first, (st, pos) = engine.device_mt19937_words(seeds=42, n=1100, skip=5, device=DEV, return_state=True)
    rest, (st2, pos2) = engine.device_mt19937_words(state=(st, pos), n=1900, device=DEV, return_state=True)
    assert np.array_equal(np.concatenate([u32(first)[0], u32(rest)[0]]), long_walk)
    _, end = randn_ref.mt19937_words(42, 3000, skip=5)
    assert int(pos2[0]) == end.pos and np.array_equal(u32(st2)[0], end.state)
    # an explicit host-side state (numpy words, int position) gets in the same way
    _, mid = randn_ref.mt19937_words(42, 1100, skip=5)
    again = engine.device_mt19937_words(state=(mid.state, mid.pos), n=1900, device=DEV)
    assert np.array_equal(u32(again), u32(rest))


def test_words_many_streams_equal_single_streams():
    seeds = [1000 + 7 * k for k in range(300)]
    many, (st, pos) = engine.device_mt19937_words(seeds=seeds, n=700, skip=3, device=DEV, return_state=True)
    many, st, pos = u32(many), u32(st), pos.cpu().numpy()
    for k in range(300):
        one, (st1, pos1) = engine.device_mt19937_words(seeds=seeds[k], n=700, skip=3, device=DEV, return_state=True)
        assert np.array_equal(u32(one)[0], many[k]) and np.array_equal(u32(st1)[0], st[k]) and int(pos1[0]) == pos[k]
    for k in (0, 1, 63, 64, 150, 299):           # and they are the yardstick's
        want, _ = randn_ref.mt19937_words(seeds[k], 700, skip=3)
        assert np.array_equal(many[k], want), k


# ------------------------------------------------------------------------------------------------ transform
def _normal_from_words(words, A, B, E, out=None, strides=None):
    """dt_rng_normal_from_words on host words [S, row]"""
    lib = _hip.load()
    w = torch.from_numpy(np.ascontiguousarray(words, dtype=np.uint32).view(np.int32)).to(DEV)
    S, pitch = w.shape
    if out is None:
        out = torch.empty(S, A * B, E, dtype=torch.float32, device=DEV)
        strides = (A * B * E, B * E, E)
    with torch.cuda.device(DEV):
        _hip.check(lib.dt_rng_normal_from_words(_hip.ptr(w), pitch, S, A, B, E, _hip.ptr(out), *strides, _hip.stream_ptr()),
                   "dt_rng_normal_from_words")
    return out


def test_transform_on_crafted_words():
    u1 = [0, 1, 2 ** 23, 2 ** 24 - 1]
    u2 = [k * 2 ** 21 for k in range(8)] + [2 ** 24 - 1]      # theta on the octant boundaries, then just below 2 pi
    pairs = [(a, b) for a in u1 for b in u2]                  # 36 pairs -> 5 groups of 16 words (8 pairs each), padded
    while len(pairs) % 8:
        pairs.append(pairs[-1])
    groups = []
    for g in range(len(pairs) // 8):
        chunk = pairs[8 * g:8 * g + 8]
        groups.append([p[0] for p in chunk] + [p[1] for p in chunk])
    base = np.array(groups, dtype=np.uint32).reshape(-1)
    # the high byte of a word is not part of the uniform: set it in a second copy
    for words in (base, base | np.uint32(0xAB000000)):
        E = len(words)
        got = u32(_normal_from_words(words[None], 1, 1, E))[0, 0]
        want = randn_ref.normal_from_words(words, E)
        assert np.array_equal(got, want.view(np.uint32))
        assert np.isfinite(want).all()
        zeros = got[(got & 0x7FFFFFFF) == 0]
        assert len(zeros) and (zeros == 0).all()              # every zero is +0 (u1 word 0: r = sqrt(-0))


def test_transform_tail_is_resolved_per_element():
    rng = np.random.default_rng(5)
    for E in (17, 31, 40):
        words = rng.integers(0, 2 ** 32, size=(2, 3 * randn_ref.words(E)), dtype=np.uint32)
        got = u32(_normal_from_words(words, 3, 1, E))
        for s in range(2):
            for d in range(3):
                W = randn_ref.words(E)
                assert np.array_equal(got[s, d], randn_ref.normal_from_words(words[s, d * W:(d + 1) * W], E).view(np.uint32))


# ------------------------------------------------------------------------------------------------ draws
@pytest.mark.parametrize("E", ELEMENTS)
def test_draws_equal_golden_yardstick_and_torch(E):
    vec = np.load(os.path.join(GOLDEN, "torch_randn_vectors.npz"))
    got = u32(engine.device_randn(seeds=SEEDS, draws=3, E=E, device=DEV))
    for k, seed in enumerate(SEEDS):
        assert np.array_equal(got[k], vec[f"seed{seed}_E{E}"].view(np.uint32)), (seed, E)
        assert np.array_equal(got[k], randn_ref.randn_stream(seed, 3, E)[0].view(np.uint32)), (seed, E)
        if host_matches_golden():
            torch.manual_seed(seed)
            live = torch.stack([torch.randn(E) for _ in range(3)]).numpy()
            assert np.array_equal(got[k], live.view(np.uint32)), (seed, E)


def test_draws_do_not_depend_on_the_chunking():
    E, draws = 105, 11
    whole, (st, pos) = engine.device_randn(seeds=[3, 4], draws=draws, E=E, skip=9, device=DEV, return_state=True)
    lib = _hip.load()
    small = torch.empty(lib.dt_rng_workspace_bytes(2, 1, E) + 2 * 2 * randn_ref.words(E) * 4, dtype=torch.uint8, device=DEV)
    chunked, (st2, pos2) = engine.device_randn(seeds=[3, 4], draws=draws, E=E, skip=9, device=DEV, return_state=True,
                                               workspace=small)       # three draws per stream and chunk
    assert torch.equal(whole, chunked) and torch.equal(st, st2) and torch.equal(pos, pos2)
    for k, seed in enumerate((3, 4)):
        stream = randn_ref.Stream(seed)
        stream.skip(9)
        want, end = randn_ref.randn_stream(stream, draws, E)
        assert np.array_equal(u32(whole)[k], want.view(np.uint32))
        assert int(pos[k]) == end.pos and np.array_equal(u32(st)[k], end.state)


def test_strides_place_draws_and_touch_nothing_else():
    A, B, E, S = 3, 4, 20, 2
    ss, sa, sb = 1000, 25, 90            # b-major with gaps: [s][b][a] rows of 25 floats, 90 per b, 1000 per stream
    sentinel = np.float32(-777.25)
    out = torch.full((S * ss + 13,), float(sentinel), dtype=torch.float32, device=DEV)
    engine.device_randn(seeds=[5, 6], draws=(A, B), E=E, out=out, strides=(ss, sa, sb), device=DEV)
    got = out.cpu().numpy()
    want = np.full_like(got, sentinel)
    for s, seed in enumerate((5, 6)):
        ref, _ = randn_ref.randn_stream(seed, A * B, E)
        for a in range(A):
            for b in range(B):
                o = s * ss + a * sa + b * sb
                want[o:o + E] = ref[a * B + b]
    assert np.array_equal(got.view(np.uint32), want.view(np.uint32))


def test_host_state_in_and_out():
    torch.manual_seed(7)
    torch.randn(5)
    raw = torch.get_rng_state()
    want = torch.stack([torch.randn(768) for _ in range(2)])
    state_after = torch.get_rng_state()
    torch.set_rng_state(raw)
    gen = engine.HostGenerator()
    got = engine.device_randn(state=gen, draws=2, E=768, device=DEV)[0].cpu()
    assert torch.equal(torch.get_rng_state(), state_after)
    ref, _ = randn_ref.randn_stream(randn_ref.parse_state(raw.numpy()), 2, 768)
    assert np.array_equal(u32(got), ref.view(np.uint32))
    assert np.array_equal(u32(got), want.numpy().view(np.uint32))      # the host's own next two draws
    assert torch.equal(torch.randn(40), _after(state_after, 40))      # and the host goes on from there


def _after(state, n):
    keep = torch.get_rng_state()
    torch.set_rng_state(state)
    out = torch.randn(n)
    torch.set_rng_state(keep)
    return out


# ------------------------------------------------------------------------------------------------ end to end
@pytest.fixture(scope="module")
def small_model():
    from distillation_trajectories_amd.config import Config
    from distillation_trajectories_amd.models import DiffusionUNet
    from distillation_trajectories_amd.synthetic import make_model
    cfg = Config()
    cfg.image_size, cfg.timesteps = 16, 4
    return cfg, make_model(DiffusionUNet, cfg, 0.1).to(DEV)


def _both_modes(fn):
    """fn(noise) under the same generator state in both modes -> (host result, device result, states equal)"""
    torch.manual_seed(123)
    torch.randn(3)
    start = torch.get_rng_state()
    host = fn("host")
    host_state = torch.get_rng_state()
    torch.set_rng_state(start)
    dev = fn("device")
    return host, dev, torch.equal(torch.get_rng_state(), host_state)


def test_generate_samples_device_noise(small_model):
    from distillation_trajectories_amd.analysis.metrics import fid_score
    cfg, model = small_model
    host, dev, same_state = _both_modes(lambda noise: fid_score.generate_samples(model, cfg, 3, DEV, noise=noise))
    assert torch.equal(host, dev) and same_state
    fixed = torch.from_numpy(np.random.default_rng(1).standard_normal((3, 3, 16, 16)).astype(np.float32))
    host, dev, same_state = _both_modes(
        lambda noise: fid_score.generate_samples(model, cfg, 3, DEV, fixed_samples=fixed, noise=noise))
    assert torch.equal(host, dev) and same_state
    x = fixed[:2].to(DEV)
    host, dev, same_state = _both_modes(lambda noise: fid_score.p_sample_loop(model, x, cfg, noise=noise))
    assert torch.equal(host, dev) and same_state


def test_noise_switch_reads_the_environment(small_model, monkeypatch):
    from distillation_trajectories_amd.analysis.metrics import fid_score
    cfg, model = small_model
    torch.manual_seed(5)
    want = fid_score.generate_samples(model, cfg, 2, DEV)
    monkeypatch.setenv("DT_NOISE", "device")
    assert engine.noise_mode() == "device" and engine.noise_mode("host") == "host"
    torch.manual_seed(5)
    assert torch.equal(fid_score.generate_samples(model, cfg, 2, DEV), want)
    monkeypatch.setenv("DT_NOISE", "gpu")
    with pytest.raises(ValueError):
        engine.noise_mode()


def test_diffusion_p_sample_loop_device_noise(small_model):
    from distillation_trajectories_amd.utils import diffusion
    cfg, model = small_model
    params = diffusion.get_diffusion_params(8, cfg)

    def run(noise):
        img, traj = diffusion.p_sample_loop(model, (2, 3, 16, 16), 8, params, device=DEV, config=cfg, track_trajectory=True,
                                            guidance_scale=2.0, noise=noise)
        return torch.cat([img.cpu().reshape(1, -1)] + [t.reshape(1, -1) for t in traj])
    host, dev, same_state = _both_modes(run)
    assert torch.equal(host, dev) and same_state


def test_noise_table_device():
    from distillation_trajectories_amd.synthetic import noise_table
    torch.manual_seed(99)
    before = torch.get_rng_state()
    host = noise_table(42, 6, (1, 3, 16, 16), noise="host")
    dev = noise_table(42, 6, (1, 3, 16, 16), noise="device", device=DEV)
    assert torch.equal(torch.get_rng_state(), before)
    assert dev.is_cuda and dev.shape == host.shape
    ref = np.stack([randn_ref.randn_stream(42 + k, 1, 768)[0][0] for k in range(6)])
    assert np.array_equal(u32(dev).reshape(6, -1), ref.view(np.uint32))
    assert torch.equal(dev.cpu(), host)


def test_callers_of_noise_table_under_the_environment_switch(monkeypatch):
    """The callers that never pass ``noise=`` get a device table when $DT_NOISE says so: the grid driver (which uploads its
    table through pinned memory) and compare_trajectories (which moves it with .to) give the numbers of the host table."""
    from distillation_trajectories_amd.analysis import trajectory_engine
    from distillation_trajectories_amd.config import Config
    from distillation_trajectories_amd.grid import grid_metrics
    from distillation_trajectories_amd.models import DiffusionUNet
    from distillation_trajectories_amd.synthetic import make_model, noise_table
    cfg = Config()
    cfg.image_size, cfg.timesteps = 16, 4
    teacher, student = make_model(DiffusionUNet, cfg, 0.1).to(DEV), make_model(DiffusionUNet, cfg, 0.05).to(DEV)
    scales = [1.0, 3.0]

    def run():
        trajectory_engine._TEACHER_CACHE.clear()
        torch.manual_seed(17)
        grid = grid_metrics(teacher, [student], cfg, scales, num_samples=3, rank=0, world=1)
        cmp = trajectory_engine.compare_trajectories(teacher, student, cfg, guidance_scales=scales, size_factor=0.05,
                                                     num_samples=3)
        return grid, cmp["student_metrics"], torch.get_rng_state()

    monkeypatch.delenv("DT_NOISE", raising=False)
    grid_h, cmp_h, state_h = run()
    monkeypatch.setenv("DT_NOISE", "device")
    with torch.cuda.device(DEV):
        assert noise_table(42, 2, (1, 3, 16, 16)).is_cuda          # the switch does reach callers that pass no keyword
    grid_d, cmp_d, state_d = run()
    assert torch.equal(state_h, state_d)
    for gs in scales:
        for k, v in cmp_h[gs].items():
            assert np.array_equal(np.float64(v), np.float64(cmp_d[gs][k]), equal_nan=True), (gs, k)
        for k, v in grid_h[0][gs].items():
            assert np.array_equal(np.float64(v), np.float64(grid_d[0][gs][k]), equal_nan=True), (gs, k)


# ------------------------------------------------------------------------------------------------ arguments
def test_bad_arguments_return_their_status():
    lib = _hip.load()
    sentinel = 3.5
    out = torch.full((4, 64), sentinel, dtype=torch.float32, device=DEV)
    words = torch.full((4, 64), 77, dtype=torch.int32, device=DEV)
    seeds = torch.tensor([1, 2], dtype=torch.int64, device=DEV)
    ws = torch.zeros(1 << 16, dtype=torch.uint8, device=DEV)
    p, sp = _hip.ptr, _hip.stream_ptr()
    DT_E_NULL, DT_E_ARG, DT_E_WORKSPACE = -1, -3, -4

    def randn(S=2, skip=0, A=1, B=1, E=16, ws_bytes=ws.numel(), seeds_p=p(seeds)):
        return lib.dt_rng_randn(seeds_p, None, None, S, skip, A, B, E, p(out), 64, 16, 16, None, None, p(ws), ws_bytes, sp)

    with torch.cuda.device(DEV):
        assert lib.dt_rng_workspace_bytes(2, 1, 15) == 0 and lib.dt_rng_workspace_bytes(2, -1, 16) == 0
        need = lib.dt_rng_workspace_bytes(2, 1, 16)
        assert need == 2 * 625 * 4 + 2 * 16 * 4
        assert randn(E=15) == DT_E_ARG
        assert randn(A=-1) == DT_E_ARG and randn(B=-2) == DT_E_ARG and randn(skip=-1) == DT_E_ARG and randn(S=0) == DT_E_ARG
        assert randn(ws_bytes=need - 1) == DT_E_WORKSPACE
        assert randn(seeds_p=None) == DT_E_NULL
        assert lib.dt_rng_mt19937_words(p(seeds), None, None, 2, 0, -1, p(words), 64, None, None, sp) == DT_E_ARG
        assert lib.dt_rng_mt19937_words(p(seeds), None, None, 2, 0, 65, p(words), 64, None, None, sp) == DT_E_ARG
        assert lib.dt_rng_mt19937_words(p(seeds), None, None, 2, 0, 8, p(words), 64, p(words), None, sp) == DT_E_NULL
        assert lib.dt_rng_normal_from_words(p(words), 64, 2, 1, 1, 15, p(out), 64, 16, 16, sp) == DT_E_ARG
        assert lib.dt_rng_normal_from_words(p(words), 64, 2, -1, 1, 16, p(out), 64, 16, 16, sp) == DT_E_ARG
        assert lib.dt_rng_normal_from_words(p(words), 64, 2, 5, 1, 16, p(out), 64, 16, 16, sp) == DT_E_ARG      # pitch 64 < 80
        assert randn(ws_bytes=need) == 0                       # the minimum is enough
    torch.cuda.synchronize()
    assert (words == 77).all()                                 # nothing was launched by the refused calls
    got = out.cpu().numpy()
    assert (got[2:] == sentinel).all() and (got[:2, 16:] == sentinel).all()
    for k in range(2):
        assert np.array_equal(got[k, :16].view(np.uint32), randn_ref.randn_stream(k + 1, 1, 16)[0][0].view(np.uint32))
    with pytest.raises(_hip.HipLibraryError):
        engine.device_randn(seeds=1, draws=1, E=15, device=DEV)
    with pytest.raises(ValueError):
        engine.device_randn(seeds=1, draws=(2, 2), E=16, out=out, strides=(0, 300, 16), device=DEV)     # 332 > 256 floats
