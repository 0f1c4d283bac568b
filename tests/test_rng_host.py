"""The float32 yardstick of the device RNG (tests/randn_ref.py) against the torch CPU generator: recorded vectors, live
``torch.randn``, the 5056-byte generator state both ways, and the words-per-draw rule.  Every comparison is of bits."""
import ctypes
import json
import os
import re
import subprocess

import numpy as np
import pytest
import torch

import randn_ref
from distillation_trajectories_amd import _hip, engine

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
with open(os.path.join(GOLDEN, "torch_randn_vectors.json")) as _f:
    META = json.load(_f)
SEEDS, ELEMENTS, DRAWS = META["seeds"], META["elements"], META["draws"]


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def test_golden_covers_the_cases():
    assert SEEDS == [0, 42, 2 ** 32 - 1, 2 ** 32 + 5] and ELEMENTS == [16, 20, 105, 768, 3072] and DRAWS == 3


def test_restatement_equals_golden():
    vec = np.load(os.path.join(GOLDEN, "torch_randn_vectors.npz"))
    for seed in SEEDS:
        for E in ELEMENTS:
            want = vec[f"seed{seed}_E{E}"]
            assert want.shape == (DRAWS, E) and want.dtype == np.float32
            got, _ = randn_ref.randn_stream(seed, DRAWS, E)
            assert np.array_equal(bits(got), bits(want)), (seed, E)


def test_restatement_equals_live_torch():
    cap = torch.backends.cpu.get_cpu_capability()
    for seed in SEEDS + [7]:
        for E in ELEMENTS + [17, 31, 4099]:
            torch.manual_seed(seed)
            want = torch.stack([torch.randn(E) for _ in range(DRAWS)]).numpy()
            got, _ = randn_ref.randn_stream(seed, DRAWS, E)
            if cap != META["cpu_capability"]:
                pytest.skip(f"live torch.randn runs the {cap} path here, the yardstick restates the recorded "
                            f"{META['cpu_capability']} one")
            assert np.array_equal(bits(got), bits(want)), (seed, E)


def test_seed_is_taken_mod_2_32():
    a, _ = randn_ref.mt19937_words(2 ** 32 + 5, 10)
    b, _ = randn_ref.mt19937_words(5, 10)
    assert np.array_equal(a, b)


def test_words_match_torch_rand():
    for seed in SEEDS:
        torch.manual_seed(seed)
        want = torch.rand(1500).numpy()
        w, _ = randn_ref.mt19937_words(seed, 1500)
        assert np.array_equal(bits(randn_ref.uniform(w)), bits(want))


def test_state_round_trip():
    for seed, E, draws in ((0, 768, 1), (42, 20, 3), (2 ** 32 - 1, 16, 39), (2 ** 32 + 5, 105, 5), (9, 624, 2)):
        torch.manual_seed(seed)
        raw0 = torch.get_rng_state().numpy()
        fresh = randn_ref.parse_state(raw0)
        assert fresh.pos == 624 and np.array_equal(fresh.state, randn_ref.init_genrand(seed))
        for _ in range(draws):
            torch.randn(E)
        raw = torch.get_rng_state().numpy()
        _, st = randn_ref.randn_stream(seed, draws, E)
        mine = randn_ref.parse_state(raw)
        assert mine.pos == st.pos and np.array_equal(mine.state, st.state), (seed, E)
        assert np.array_equal(randn_ref.write_state(raw0, st), raw), (seed, E)
        # an advanced state written back: torch continues from it
        more, st2 = randn_ref.randn_stream(st, 2, E)
        torch.manual_seed(12345)
        torch.set_rng_state(torch.from_numpy(randn_ref.write_state(raw0, st2)))
        nxt_t = torch.rand(700).numpy()
        want_state_after = torch.get_rng_state().numpy()
        w, st3 = randn_ref.mt19937_words(st2, 700)
        assert np.array_equal(bits(randn_ref.uniform(w)), bits(nxt_t)), (seed, E)
        assert np.array_equal(randn_ref.write_state(raw0, st3), want_state_after)
        # and the host's own continuation is the yardstick's
        torch.set_rng_state(torch.from_numpy(raw))
        host_more = torch.stack([torch.randn(E) for _ in range(2)]).numpy()
        if torch.backends.cpu.get_cpu_capability() == META["cpu_capability"]:
            assert np.array_equal(bits(more), bits(host_more)), (seed, E)


def test_state_keeps_seed_and_cache():
    torch.manual_seed(7)
    torch.randn(5)                      # the scalar path: leaves a cached normal sample behind the state words
    raw = torch.get_rng_state().numpy()
    assert raw[5016:].any()
    st = randn_ref.parse_state(raw)
    out = randn_ref.write_state(raw, st)
    assert np.array_equal(out, raw)
    st.words(1000)
    out = randn_ref.write_state(raw, st)
    assert np.array_equal(out[:8], raw[:8]) and np.array_equal(out[12:16], raw[12:16])
    assert np.array_equal(out[5016:], raw[5016:])


@pytest.mark.parametrize("E", [16, 17, 20, 31, 32, 105, 768, 769, 3072])
def test_word_count_rule(E):
    assert randn_ref.words(E) == (E if E % 16 == 0 else E + 16)
    torch.manual_seed(11)
    torch.randn(E)
    torch.randn(E)
    raw = torch.get_rng_state().numpy()
    st = randn_ref.Stream(11)
    st.skip(2 * randn_ref.words(E))
    got = randn_ref.parse_state(raw)
    assert got.pos == st.pos and np.array_equal(got.state, st.state)
    # the second draw starts at word words(E) of the stream
    w, _ = randn_ref.mt19937_words(11, randn_ref.words(E), skip=randn_ref.words(E))
    two, _ = randn_ref.randn_stream(11, 2, E)
    assert np.array_equal(bits(randn_ref.normal_from_words(w, E)), bits(two[1]))


def test_fewer_than_16_elements_is_refused():
    with pytest.raises(ValueError):
        randn_ref.words(15)


# ------------------------------------------------------------------------------------------------ library and host helpers
def test_library_exports_and_binding_lists_what_the_header_declares():
    from distillation_trajectories_amd.csrc.build import LIB, build
    lib_path = build() if not os.path.exists(LIB) else LIB
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    text = re.sub(r"/\*.*?\*/", "", open(os.path.join(root, "include", "dt_hip_rng.h")).read(), flags=re.S)
    names = sorted(set(re.findall(r"\b(dt_[a-z0-9_]+)\s*\(", text)))
    assert names == ["dt_rng_mt19937_words", "dt_rng_normal_from_words", "dt_rng_randn", "dt_rng_workspace_bytes"]
    assert sorted(_hip.RNG_SIGNATURES) == names
    out = subprocess.run(["nm", "-D", "--defined-only", lib_path], capture_output=True, text=True, check=True).stdout
    exported = set(re.findall(r" T (dt_[a-z0-9_]+)", out))
    assert not [n for n in names if n not in exported]
    lib = _hip.load(lib_path)
    assert lib.dt_abi_version() == _hip.ABI_VERSION == 6
    for n in names:                                       # one ctypes argument per parameter of the declaration
        decl = re.search(rf"\b{n}\s*\((.*?)\);", text, flags=re.S).group(1)
        assert len(_hip.RNG_SIGNATURES[n][1]) == len(decl.split(",")), n
    # the queries and the argument checks run without a device
    assert lib.dt_rng_workspace_bytes(2, 1, 16) == 2 * 625 * 4 + 2 * 16 * 4
    assert lib.dt_rng_workspace_bytes(1, 10 ** 12, 768) <= 625 * 4 + (64 << 20)          # bounded whatever the draw count
    assert lib.dt_rng_workspace_bytes(1, 1, 15) == 0
    assert lib.dt_rng_randn(None, None, None, 1, 0, 1, 1, 16, None, 0, 0, 0, None, None, None, 0, None) == -1     # DT_E_NULL
    assert lib.dt_rng_normal_from_words(None, 0, 1, 1, 1, 15, None, 0, 0, 0, None) == -3                          # DT_E_ARG
    # the limits of one launch: B < 2^31, at most 2^30 wave units
    assert lib.dt_rng_normal_from_words(None, 0, 1, 1, 2 ** 31, 16, None, 0, 0, 0, None) == -3
    assert lib.dt_rng_normal_from_words(None, 0, 1, 2 ** 30 + 1, 1, 16, None, 0, 0, 0, None) == -3
    assert lib.dt_rng_normal_from_words(None, 0, 2 ** 20, 1, 1, 2 ** 18, None, 0, 0, 0, None) == -3       # S * units(E) = 2^31
    assert lib.dt_rng_normal_from_words(None, 0, 1, 2 ** 30, 1, 16, None, 0, 0, 0, None) == -1            # within: then DT_E_NULL
    seeds = (ctypes.c_uint64 * 1)(5)       # (never read: these calls end in the argument checks)
    assert lib.dt_rng_randn(seeds, None, None, 2 ** 20, 0, 1, 1, 2 ** 18, None, 0, 0, 0, None, None, None, 0, None) == -3
    assert lib.dt_rng_randn(seeds, None, None, 1, 0, 1, 2 ** 31, 16, None, 0, 0, 0, None, None, None, 0, None) == -3
    # no draws and no end state asked for: nothing to do, no workspace needed
    assert lib.dt_rng_randn(seeds, None, None, 1, 100, 0, 3, 16, None, 0, 0, 0, None, None, None, 0, None) == 0
    assert lib.dt_rng_randn(seeds, None, None, 1, 0, 2, 0, 16, None, 0, 0, 0, None, None, None, 0, None) == 0
    with pytest.raises(_hip.HipLibraryError, match="at least 16 elements"):
        engine.device_randn(seeds=1, draws=1, E=15)


def test_host_generator_reads_and_writes_the_state():
    torch.manual_seed(7)
    fresh = engine.HostGenerator()
    assert fresh.pos == 624 and np.array_equal(fresh.words, randn_ref.init_genrand(7))
    torch.randn(5)
    torch.randn(100)
    raw = torch.get_rng_state()
    gen = engine.HostGenerator()
    mine = randn_ref.parse_state(raw.numpy())
    assert gen.pos == mine.pos and np.array_equal(gen.words, mine.state)
    assert np.array_equal(gen.state_bytes(gen.words, gen.pos), raw.numpy())
    mine.words(2000)
    want = randn_ref.write_state(raw.numpy(), mine)
    assert np.array_equal(gen.state_bytes(mine.state, mine.pos), want)
    gen.write(torch.from_numpy(mine.state.view(np.int32)), torch.tensor([mine.pos], dtype=torch.int32))
    assert np.array_equal(torch.get_rng_state().numpy(), want)
    torch.set_rng_state(raw)
    torch.rand(2000)
    assert np.array_equal(torch.get_rng_state().numpy(), want)


def test_noise_switch_defaults_to_host(monkeypatch):
    monkeypatch.delenv("DT_NOISE", raising=False)
    assert engine.noise_mode() == "host" and engine.noise_mode("device") == "device"
    monkeypatch.setenv("DT_NOISE", "device")
    assert engine.noise_mode() == "device" and engine.noise_mode("host") == "host"
    with pytest.raises(ValueError):
        engine.noise_mode("cuda")
    from distillation_trajectories_amd.synthetic import noise_table, seeded_noise
    torch.manual_seed(3)
    before = torch.get_rng_state()
    table = noise_table(42, 3, (1, 3, 4, 4), noise="host")
    assert torch.equal(torch.get_rng_state(), before) and not table.is_cuda
    assert torch.equal(table[2], seeded_noise(44, (1, 3, 4, 4)))
