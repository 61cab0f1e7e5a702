"""Fixture of the mapped interface-accuracy tests, from the NumPy restatement alone (tests/interface_mapped_ref.py):

    python tests/golden/make_goldens_interface_mapped.py      # -> tests/golden/interface_mapped_cases.npz

The cases are ``interface_mapped_ref.cases()``: cut from the complexes of tests/golden/sasa_cases.npz and rebuilt by the tests, so no
coordinate is copied.  Per case and coverage mode (``<case>.<ignore | penalise>``), from the restatement:

* every output of ``interface_mapped_ref.mapped_all`` in ascending order, with ``n_covered`` and ``n_reference``;
* ``<...>.<float output>.yard``: its largest change when every sum over atoms runs in descending order instead - what
  ``interface_ref.bound`` reads;
* asserted, not stored: the smallest |d^2 - c^2| / c^2 over every tested atom pair and both cutoffs (taken on the far-point model, which
  tests every pair the mapped contract tests) is above 1e-9, and the relative eigenvalue gap of every superposition above 1e-6: no
  integer and no status bit hangs on rounding.
"""
from __future__ import annotations

import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))

import interface_mapped_ref as mr  # noqa: E402
import interface_ref as ir  # noqa: E402

MARGIN, GAP = 1e-9, 1e-6
LIMIT = 1 << 20  # the repository's size limit of a committed file


def record(fix, name, case, coverage):
    key = f"{name}.{coverage}"
    out = mr.mapped_all(case["xa"], case["xb"], case["sides"], case["m"], coverage=coverage, **mr.case_kw(case))
    other = mr.mapped_all(case["xa"], case["xb"], case["sides"], case["m"], coverage=coverage, descending=True, **mr.case_kw(case))
    assert not np.any(out["status"] & ir.DEGENERATE) and all(g > GAP for g in out["gaps"]), (key, out["gaps"])
    for k in mr.INT_OUTPUTS + ir.ROW_OUTPUTS:
        assert np.array_equal(out[k], other[k]), (key, k)  # (no integer depends on the order)
        fix[f"{key}.{k}"] = np.asarray(out[k]).astype(np.bool_ if k == "interface_rows" else np.int32)
    for k in ir.FLOAT_OUTPUTS:
        fix[f"{key}.{k}"] = np.asarray(out[k], dtype=np.float64)
        both = np.isfinite(out[k]) & np.isfinite(other[k])
        assert np.array_equal(np.isfinite(out[k]), np.isfinite(other[k])), (key, k)
        fix[f"{key}.{k}.yard"] = np.float64(np.max(np.abs(out[k] - other[k])[both], initial=0.0))
    fix[f"{key}.n_covered"], fix[f"{key}.n_reference"] = np.int32(out["n_covered"]), np.int32(out["n_reference"])
    print(f"{key}: mode {case['mode']}, rows {len(case['xb'])} <- {len(case['xa'])}, covered {out['n_covered']}, native {out['n_native'].tolist()}, "
          f"model {out['n_model'].tolist()}, shared {out['n_shared'].tolist()}, interface rows {out['n_interface_rows'].tolist()} (covered "
          f"{out['n_interface_covered'].tolist()}), status {out['status'].tolist()}, irmsd {np.round(out['irmsd'], 3).tolist()}, lrmsd "
          f"{np.round(out['lrmsd'], 3).tolist()}, dockq {np.round(out['dockq'], 3).tolist()}", flush=True)


def main():
    fix, names = {}, []
    for name, case in mr.cases().items():
        xf, rows, mask = mr.far_point_model(case["xa"], case["xb"], case["m"], res_mask_a=case["res_mask_a"])
        margin = ir.interface_all(xf, case["xb"], case["sides"], case["mode"], res_mask_a=rows, mask_a=mask)["margin"]
        assert margin > MARGIN, (name, margin)
        for coverage in ("ignore", "penalise"):
            record(fix, name, case, coverage)
        names.append(name)
    fix["cases"] = np.array(names)
    path = os.path.join(HERE, "interface_mapped_cases.npz")
    np.savez_compressed(path, **fix)
    assert os.path.getsize(path) < LIMIT, os.path.getsize(path)
    print(f"{os.path.getsize(path) / 1024:.0f} KB")


if __name__ == "__main__":
    main()
