"""Records ``torch.randn`` of the CPU generator as tests/golden/torch_randn_vectors.npz (+ .json): for every seed and element
count E below, three consecutive fp32 draws of E elements right after ``torch.manual_seed(seed)``.  The json names the torch
version and the CPU capability the vectors were recorded with (the vectorised Box-Muller path is per capability).

    python tests/golden/make_golden_randn.py
"""
import json
import os

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
SEEDS = [0, 42, 2 ** 32 - 1, 2 ** 32 + 5]
ELEMENTS = [16, 20, 105, 768, 3072]
DRAWS = 3


def key(seed, E):
    return f"seed{seed}_E{E}"


def main():
    arrays = {}
    for seed in SEEDS:
        for E in ELEMENTS:
            torch.manual_seed(seed)
            arrays[key(seed, E)] = torch.stack([torch.randn(E) for _ in range(DRAWS)]).numpy()
    np.savez(os.path.join(HERE, "torch_randn_vectors.npz"), **arrays)
    meta = {"torch_version": torch.__version__, "cpu_capability": torch.backends.cpu.get_cpu_capability(),
            "seeds": SEEDS, "elements": ELEMENTS, "draws": DRAWS, "dtype": "float32",
            "layout": "seed{seed}_E{E}: [draws, E], consecutive torch.randn(E) after torch.manual_seed(seed)"}
    with open(os.path.join(HERE, "torch_randn_vectors.json"), "w") as f:
        json.dump(meta, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
