"""Fixture of the sample-selection tests, captured from the reference (this container only):

    python tests/golden/make_goldens_selection.py      # -> tests/golden/selection_cases.npz

Per case (tests/selection_ref.py: CASES) synthetic float32 backbones at realistic magnitudes - a chain walk tens of Angstrom from the
origin, samples scattered around it - widened to float64 and passed through ``evaluation.utils.sample_selection``:
``get_mean_coordinates``, ``get_median_coordinates``, ``gaussian_density_estimation``, ``get_mode_index`` and ``get_closest_index``
(against mean and median).  Also recorded:

* ``perm_diff``: the largest difference of the reference's median against itself over three permutations of the sample order - the
  yardstick of the coordinate tolerance;
* ``gaps``: for mode, mean_closest and median_closest the distance between the best and the second-best sample relative to the
  criterion's value; asserted >= 1e-6 here so that index parity is decidable (seeds are chosen for that).

The single-sample case records no median (the reference returns NaN) and no gaps.
"""
from __future__ import annotations

import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(HERE))

import refharness as rh  # noqa: E402

rh.install_stubs()
from evaluation.utils import sample_selection as ss  # noqa: E402

import selection_ref as sr  # noqa: E402

# name: (S, N, diffused regions as (first row, length), seed, shift of the last sample in Angstrom)
SPEC = {
    "s5_two_chains": (5, 19, ((3, 5), (11, 7)), 11, 0.0),
    "s7_l40": (7, 45, ((2, 40),), 12, 0.0),
    "s64_l21": (64, 25, ((1, 21),), 13, 0.0),
    "s33_l9": (33, 14, ((4, 9),), 14, 0.0),
    "s3_l1": (3, 6, ((2, 1),), 15, 0.0),
    "s1_l4": (1, 9, ((3, 4),), 16, 0.0),
    "s5_outlier": (5, 15, ((2, 10),), 17, 6.0),
}


def backbones(s, n, seed, shift):
    """[S,N,5,3] float32: atom37 columns N, CA, C, CB, O of S samples around one chain walk."""
    rng = np.random.default_rng(seed)
    steps = rng.normal(size=(n, 3))
    ca = np.array([31.0, -47.0, 58.0]) + np.cumsum(3.8 * steps / np.linalg.norm(steps, axis=-1, keepdims=True), axis=0)
    atoms = ca[:, None, :] + np.concatenate([1.46 * rng.normal(size=(n, 1, 3)) / np.sqrt(3), np.zeros((n, 1, 3)),
                                             1.52 * rng.normal(size=(n, 1, 3)) / np.sqrt(3), 1.53 * rng.normal(size=(n, 1, 3)) / np.sqrt(3),
                                             2.4 * rng.normal(size=(n, 1, 3)) / np.sqrt(3)], axis=1)
    x = atoms[None] + 1.5 * rng.normal(size=(s, n, 1, 3)) + 0.3 * rng.normal(size=(s, n, 5, 3))
    if shift:
        x[-1] += shift * np.array([2.0, -1.0, 2.0]) / 3.0
    return x.astype(np.float32)


def region_dict(bb, regions):
    """{chain id: [S,L_c,4,3] float64} as get_selected_models builds it, in BACKBONE_ATOMS order."""
    cols = [{0: 0, 1: 1, 2: 2, 4: 4}[c] for c in sr.BACKBONE_COLUMNS]  # (the fixture holds atom37 columns 0 .. 4 as they are)
    return {chr(ord("A") + i): bb[:, a:a + n][:, :, cols].astype(np.float64) for i, (a, n) in enumerate(regions)}


def gap(values, best_is_max):
    v = np.sort(np.asarray(values))
    return float((v[-1] - v[-2]) / abs(v[-1])) if best_is_max else float((v[1] - v[0]) / abs(v[0]))


def main():
    out = {}
    for name, (s, n, regions, seed, shift) in SPEC.items():
        bb = backbones(s, n, seed, shift)
        mask = np.zeros(n, dtype=np.float32)
        for a, ln in regions:
            mask[a:a + ln] = 1
        coords = region_dict(bb, regions)
        cat = lambda d: np.concatenate(list(d.values()), axis=0)  # noqa: E731
        mean = ss.get_mean_coordinates(coords)
        flat = ss.flatten_diffused_region_coords(coords)
        density = ss.gaussian_density_estimation(flat)
        out.update({f"{name}.bb": bb, f"{name}.mask": mask, f"{name}.mean": cat(mean), f"{name}.density": density,
                    f"{name}.mode": np.int64(ss.get_mode_index(coords)),
                    f"{name}.mean_closest": np.int64(ss.get_closest_index(coords, mean))})
        if s == 1:
            out[f"{name}.perm_diff"] = np.float64(0.0)
            continue
        median = ss.get_median_coordinates(coords)
        assert np.isfinite(cat(median)).all()
        perm_diff = 0.0
        for k in range(3):
            perm = np.random.default_rng(1000 + k).permutation(s)
            again = ss.get_median_coordinates({c: v[perm] for c, v in coords.items()})
            perm_diff = max(perm_diff, float(np.abs(cat(again) - cat(median)).max()))
        x = np.concatenate(list(coords.values()), axis=1)
        gaps = np.array([gap(density, True), gap(sr.closest_distances(x, cat(mean)), False), gap(sr.closest_distances(x, cat(median)), False)])
        assert (gaps >= 1e-6).all(), (name, gaps)
        out.update({f"{name}.median": cat(median), f"{name}.median_closest": np.int64(ss.get_closest_index(coords, median)),
                    f"{name}.perm_diff": np.float64(perm_diff), f"{name}.gaps": gaps})
        print(f"{name}: S = {s}, L = {int(mask.sum())}, perm_diff = {perm_diff:.2e}, gaps = {gaps}")
    assert set(SPEC) == set(sr.CASES)
    np.savez_compressed(os.path.join(HERE, "selection_cases.npz"), **out)


if __name__ == "__main__":
    main()
