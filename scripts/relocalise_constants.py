"""Measures, on the CPU, the constants in tests/relocalise_scenes.py that tests/test_gpu_relocalise.py asserts against (no GPU):

  * per seed of HYP_SEEDS (N = 65, H = 256) and for the end-to-end scene (N = 257): how many hypotheses the reference solves
    differently in float64 and in longdouble, and the largest float64-vs-longdouble pose difference among the 95 % kept;
  * the error of the reference's selected end-to-end pose against the sequence's ground truth.

Run from the repository root:  python scripts/relocalise_constants.py [seed ...]   (other seeds: to choose new ones)
"""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "tests")):
    if p not in sys.path:
        sys.path.insert(0, p)

import relocalise_scenes as t  # noqa: E402  (the scenes and the ranking are the tests' own)


def measure(scene, seed):
    ref = scene.reference(seed=seed)
    disc = t.hypothesis_discrepancies(scene, ref)
    n_inf = int(np.sum(~np.isfinite(disc)))
    n_out = int(np.floor(t.LEFT_OUT * len(disc)))
    kept = np.sort(disc)[: len(disc) - n_out]
    return ref, n_inf, n_out, float(kept.max())


def main():
    seeds = [int(s) for s in sys.argv[1:]] or list(t.HYP_SEEDS)
    s65 = t.Scene(65)
    for seed in seeds:
        ref, n_inf, n_out, worst = measure(s65, seed)
        print(f"N=65 seed={seed}: candidates={ref['n_candidates']} valid={ref['n_valid_hypotheses']} not finite={n_inf} "
              f"(cap {n_out}) discrepancy of the kept={worst:.6e} best inliers={ref['n_inliers']}")
    s257 = t.Scene(257)
    ref, n_inf, n_out, worst = measure(s257, t.PARAMS["seed"])
    print(f"N=257 seed={t.PARAMS['seed']}: candidates={ref['n_candidates']} valid={ref['n_valid_hypotheses']} not finite={n_inf} "
          f"(cap {n_out}) discrepancy of the kept={worst:.6e} found={ref['found']} inliers={ref['n_inliers']} rms={ref['rms_px']:.4f}")
    er = float(np.max(np.abs(ref["r"] - s257.seq.truth_r[t.FRAME])))
    eq = float(np.max(np.abs(ref["q"] - s257.seq.truth_q[t.FRAME])))
    print(f"N=257 reference pose error against the truth: r {er:.6e}  q {eq:.6e}")


if __name__ == "__main__":
    main()
