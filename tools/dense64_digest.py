"""SHA-256 of what the two fp64 dense stages compute on seeded inputs: engine.device_pca, engine.device_pca_project and
engine.device_fid at small shapes that touch every edge of csrc/dt_dense64.h (one tile, one row into the next tile, three
tile rows, a last LDS stage of one quad, padded E, M M^T and M^T M, a shared 2-D set, strided views, a NaN in one problem
of three); after those, engine.device_fid_cov, engine.device_quality and engine.device_quality_stream (csrc/dt_fid.hip,
csrc/dt_quality.hip, csrc/dt_quality_stream.hip and what they share in csrc/dt_dense64.h and csrc/dt_quality_math.h) at
shapes that touch a partial and a mirrored covariance tile, two and three row slabs, a mean chunk crossed in one set, zero
pivots, subset tables, partial panels and tiles, a refill of the selection buffer at k = 5 and at its tightest fit
k = 1023, a shared 2-D teacher, strided views, a NaN in either set, and last one whole-matrix case whose two sets come from
one pool (non-zero counts).  One line per output tensor, status words included.
Two builds that print the same lines compute the same bits.

    python tools/dense64_digest.py
"""
import hashlib
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from distillation_trajectories_amd import engine  # noqa: E402

DEV = torch.device("cuda:0")
PCA_FIELDS = ("mean", "components", "scores", "singular_values", "explained_variance", "explained_variance_ratio", "status")
PCA_SHAPES = [(64, 0, 64, 1, 2), (33, 32, 36, 2, 3), (65, 64, 20, 2, 3), (26, 26, 675, 2, 16)]      # n_a, n_b, E, P, k
FID_SHAPES = [(65, 64, 2, 80), (64, 65, 2, 80), (129, 63, 1, 36), (64, 64, 1, 2048), (2, 50, 1, 2048)]  # n_a, n_b, P, D
FID_COV_SHAPES = [(65, 70, 2, 36), (1100, 530, 2, 68), (20, 300, 1, 68)]                               # n_a, n_b, P, D
QUALITY_FIELDS = ("kid", "kid_subsets", "counts", "precision", "recall", "density", "coverage", "status", "radii_a",
                  "radii_b")
QUALITY_SHAPES = [(65, 64, 2, 36, 3), (64, 65, 2, 36, 3)]                                              # n_a, n_b, P, D, k


def line(name, t):
    t = t.contiguous().cpu()
    print(f"{name:52s} {hashlib.sha256(t.numpy().tobytes()).hexdigest()}", flush=True)


def walk(seed, n, P, E, scale=1.0):
    """step-major random walks [n, P, E] fp32 on a common offset, from a CPU generator"""
    g = torch.Generator().manual_seed(seed)
    return (torch.randn(n, P, E, generator=g, dtype=torch.float64).cumsum(0) * scale + 5.0).float()


def features(seed, P, n, D, shift=0.0):
    """feature-like sets [P, n, D] fp32: a common offset per column, a decaying spectrum, from a CPU generator"""
    g = torch.Generator().manual_seed(seed)
    coeff = torch.randn(P, n, D, generator=g, dtype=torch.float64) * torch.rsqrt(1.0 + torch.arange(D, dtype=torch.float64))
    base = 0.4 * (1.0 + torch.rand(D, generator=g, dtype=torch.float64)) + shift
    return (base + 0.15 * coeff).float()


def pca_lines(tag, a, k, b=None):
    r = engine.device_pca(a, k, b)
    for f in PCA_FIELDS:
        line(f"pca {tag} {f}", r[f])
    if (r["status"] == 0).all():
        line(f"pca {tag} project", engine.device_pca_project(a, r["mean"], r["components"], b))
        line(f"pca {tag} project shared", engine.device_pca_project(a, r["mean"][0], r["components"][0], b))


def fid_lines(tag, a, b):
    r = engine.device_fid(a, b)
    for f in ("fid", "parts", "status"):
        line(f"fid {tag} {f}", r[f])


def fid_cov_lines(tag, a, b):
    r = engine.device_fid_cov(a, b)
    for f in ("fid", "parts", "status"):
        line(f"fid_cov {tag} {f}", r[f])


def quality_lines(tag, a, b, k, subsets=None):
    r = engine.device_quality(a, b, k=k, subsets=subsets, radii=True)
    for f in QUALITY_FIELDS:
        line(f"quality {tag} {f}", r[f])


def stream_lines(tag, a, b, k, panel_rows):
    r = engine.device_quality_stream(a, b, k=k, radii=True, panel_rows=panel_rows)
    for f in QUALITY_FIELDS:
        line(f"quality_stream {tag} {f}", r[f])


def subset_tables(seed, S, m, n_a, n_b):
    """(idx_a, idx_b) int64 [S, m]: m distinct rows per subset, from a CPU generator"""
    g = torch.Generator().manual_seed(seed)
    return tuple(torch.stack([torch.randperm(n, generator=g)[:m] for _ in range(S)]) for n in (n_a, n_b))


def main():
    for n_a, n_b, E, P, k in PCA_SHAPES:
        a = walk(100 + n_a, n_a, P, E).to(DEV)
        b = walk(200 + n_b, n_b, P, E, 0.8).to(DEV) if n_b else None
        pca_lines(f"{n_a}+{n_b}x{E} P{P} k{k}", a, k, b)
    wide_a, wide_b = walk(133, 33, 4, 44).to(DEV), walk(232, 32, 4, 44, 0.8).to(DEV)
    va, vb = wide_a[:, ::2, 4:40], wide_b[:, ::2, 4:40]                      # every other problem, 36 of 44 columns
    assert not va.is_contiguous() and va.data_ptr() % 16 == 0
    pca_lines("33+32x36 P2 k3 strided", va, 3, vb)
    a, b = walk(301, 33, 3, 36), walk(302, 32, 3, 36, 0.8)
    a[7, 1, 21] = float("nan")
    pca_lines("33+32x36 P3 k3 nan in 1", a.to(DEV), 3, b.to(DEV))

    for n_a, n_b, P, D in FID_SHAPES:
        fid_lines(f"{n_a}x{n_b} P{P} D{D}", features(400 + n_a, P, n_a, D).to(DEV),
                  features(500 + n_b, P, n_b, D, 0.01).to(DEV))
    teacher, students = features(601, 1, 65, 80)[0].to(DEV), features(602, 3, 64, 80, 0.01).to(DEV)
    fid_lines("65x64 P3 D80 shared 2-D teacher", teacher, students)
    wide_a = torch.zeros(65, 88, device=DEV)
    wide_a[:, :80] = teacher
    wide_b = torch.full((6, 67, 88), float("nan"), device=DEV)
    wide_b[::2, 1:65, 4:84] = students
    va, vb = wide_a[:, :80], wide_b[::2, 1:65, 4:84]
    assert not va.is_contiguous() and not vb.is_contiguous()
    fid_lines("65x64 P3 D80 strided", va, vb)
    bad = students.clone()
    bad[1, 63, 79] = float("nan")
    fid_lines("65x64 P3 D80 nan in 1", teacher, bad)

    for n_a, n_b, P, D in FID_COV_SHAPES:
        fid_cov_lines(f"{n_a}x{n_b} P{P} D{D}", features(700 + n_a, P, n_a, D).to(DEV),
                      features(800 + n_b, P, n_b, D, 0.01).to(DEV))
    fid_cov_lines("65x64 P3 D80 shared 2-D teacher", teacher, students)
    fid_cov_lines("65x64 P3 D80 strided", va, vb)
    fid_cov_lines("65x64 P3 D80 nan in 1", teacher, bad)

    for n_a, n_b, P, D, k in QUALITY_SHAPES:
        quality_lines(f"{n_a}x{n_b} P{P} D{D} k{k}", features(900 + n_a, P, n_a, D).to(DEV),
                      features(1000 + n_b, P, n_b, D, 0.01).to(DEV), k)
    quality_lines("130x70 P1 D20 k5 3 subsets of 16", features(1101, 1, 130, 20).to(DEV),
                  features(1102, 1, 70, 20, 0.01).to(DEV), 5, subset_tables(1103, 3, 16, 130, 70))
    quality_lines("65x64 P3 D80 k3 shared 2-D teacher", teacher, students, 3)
    quality_lines("65x64 P3 D80 k3 nan in 1", teacher, bad, 3)

    a, b = features(1201, 2, 130, 36).to(DEV), features(1202, 2, 70, 36, 0.01).to(DEV)
    stream_lines("130x70 P2 D36 k3 panel 64", a, b, 3, 64)
    stream_lines("130x70 P2 D36 k3 panel default", a, b, 3, None)
    a, b = features(1301, 1, 2100, 8).to(DEV), features(1302, 1, 1900, 8, 0.01).to(DEV)
    for k in (5, 1023):
        stream_lines(f"2100x1900 P1 D8 k{k} panel 256", a, b, k, 256)
    stream_lines("65x64 P3 D80 k3 shared 2-D teacher", teacher, students, 3, None)
    copies = teacher.unsqueeze(0).repeat(3, 1, 1)
    bad_a = copies.clone()
    bad_a[1, 7, 21] = float("nan")
    stream_lines("65x64 P3 D80 k3 nan in A of 1", bad_a, students, 3, None)
    stream_lines("65x64 P3 D80 k3 nan in B of 1", copies, bad, 3, None)

    # both sets from one pool (the same column offsets), so that the whole-matrix route's counts are not all zero
    pool = features(1401, 2, 135, 36)
    quality_lines("65x70 P2 D36 k3 one pool", pool[:, :65].contiguous().to(DEV), pool[:, 65:].contiguous().to(DEV), 3)


if __name__ == "__main__":
    main()
