#!/usr/bin/env python3
"""Reference vectors of the noise-prediction driver: tests/golden/reference_vectors_noise.{npz,json}.

Run from the repo root:  python tests/golden/make_golden_noise.py   (container only: imports /root/reference
through make_golden.py's stub modules; nothing of the reference is copied, only inputs / seeds / outputs).

Case: the reference's own ``analyze_noise_prediction`` (analysis/noise_prediction/noise_analysis.py:197-321) on the CPU,
teacher sf 0.5 against students sf 0.2 and sf 1.0 (``synthetic.make_model``), ``fixed_samples`` = 6 seeded images at
16 x 16 x 3, ``config.timesteps = 20``, the global generator seeded with NOISE_SEED right before each call.  Recorded:
  * the images, the 10 noise tensors (every ``torch.randn_like`` of the call, in order), the noised inputs the two models
    see (the first argument of each ``predict_noise`` call) and the fp32 coefficients (every ``torch.sqrt`` result of the
    call: sqrt(ab_t), sqrt(1 - ab_t) per timestep);
  * the returned dict, the bytes of noise_metrics_size_{sf}.txt and the console lines.
"""
import contextlib
import io
import json
import os
import sys
import tempfile

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import make_golden as mg   # noqa: E402  (registers the torchvision / umap stubs, imports the reference)

import numpy as np   # noqa: E402
import torch         # noqa: E402

import analysis.noise_prediction.noise_analysis as ref_na   # noqa: E402

from distillation_trajectories_amd.synthetic import make_model, state_dict_digest  # noqa: E402

T, B, IMAGE_SEED, NOISE_SEED = 20, 6, 321, 2024


def run_case(teacher, student, sf, images):
    c = mg.cfg(16, T)
    noise, sqrts, noised = [], [], []
    randn_like, sqrt, predict = torch.randn_like, torch.sqrt, ref_na.predict_noise

    def rec_randn_like(*a, **k):
        r = randn_like(*a, **k)
        noise.append(r.clone())
        return r

    def rec_sqrt(*a, **k):
        r = sqrt(*a, **k)
        sqrts.append(r.clone())
        return r

    def rec_predict(model, noisy_images, timesteps, device):
        if model is teacher:
            noised.append(noisy_images.clone())
        return predict(model, noisy_images, timesteps, device)

    out_dir = tempfile.mkdtemp(prefix="dt_golden_noise_")
    torch.manual_seed(NOISE_SEED)
    buf = io.StringIO()
    torch.randn_like, torch.sqrt, ref_na.predict_noise = rec_randn_like, rec_sqrt, rec_predict
    try:
        with contextlib.redirect_stdout(buf):
            res = ref_na.analyze_noise_prediction(teacher, student, c, output_dir=out_dir, size_factor=sf, fixed_samples=images)
    finally:
        torch.randn_like, torch.sqrt, ref_na.predict_noise = randn_like, sqrt, predict
    with open(os.path.join(out_dir, f"noise_metrics_size_{sf}.txt"), "rb") as f:
        txt = f.read()
    assert len(noise) == 10 and len(sqrts) == 20 and len(noised) == 10
    coef = torch.stack([torch.stack(sqrts[0::2]), torch.stack(sqrts[1::2])], dim=1)     # [10, 2] fp32
    assert coef.dtype == torch.float32
    return res, txt.decode(), buf.getvalue(), torch.stack(noise), coef, torch.stack(noised)


def main():
    out_npz, out_json = {}, {"torch": torch.__version__, "numpy": np.__version__}
    mdl = {sf: make_model(mg.ref_models.DiffusionUNet, mg.cfg(), sf) for sf in (0.5, 0.2, 1.0)}
    out_json["state_dict_sha256"] = {str(sf): state_dict_digest(m.state_dict()) for sf, m in mdl.items()}
    torch.manual_seed(IMAGE_SEED)
    images = torch.rand(B, 3, 16, 16) * 2 - 1
    out_npz["images"] = images.numpy()
    t_list = torch.linspace(0, T - 1, 10, dtype=torch.long).tolist()
    out_json.update(T=T, teacher_sf=0.5, image_seed=IMAGE_SEED, noise_seed=NOISE_SEED, timesteps=t_list, cases={})
    for sf in (0.2, 1.0):
        with torch.no_grad():
            res, txt, console, noise, coef, noised = run_case(mdl[0.5], mdl[sf], sf, images)
        if "noise" in out_npz:
            assert np.array_equal(out_npz["noise"], noise.numpy()) and np.array_equal(out_npz["coef"], coef.numpy())
            assert np.array_equal(out_npz["noised"], noised.numpy())
        out_npz["noise"], out_npz["coef"], out_npz["noised"] = noise.numpy(), coef.numpy(), noised.numpy()
        out_json["cases"][str(sf)] = dict(
            student_sf=sf, avg_mse=float(res["avg_mse"]), avg_mae=float(res["avg_mae"]),
            avg_cosine_similarity=float(res["avg_cosine_similarity"]),
            metrics_by_timestep={str(t): {k: float(v) for k, v in m.items()} for t, m in res["metrics_by_timestep"].items()},
            txt=txt, console=console)
    np.savez_compressed(os.path.join(HERE, "reference_vectors_noise.npz"), **out_npz)
    with open(os.path.join(HERE, "reference_vectors_noise.json"), "w") as f:
        json.dump(out_json, f, indent=1)
    print("wrote", len(out_npz), "arrays;", os.path.getsize(os.path.join(HERE, "reference_vectors_noise.npz")) / 1e6, "MB")


if __name__ == "__main__":
    main()
