"""Dense NumPy restatement of the interface-accuracy contract (include/fdipt.h "interface accuracy"): the contacts
across an interface in the reference and in the model, fnat, fnonnat, interface RMSD, ligand RMSD, DockQ and the status bits of one
(model, reference) pair on one interface, in float64.  Also the readers of the fixture tests/golden/interface_cases.npz
(tests/golden/make_goldens_interface.py) and the bounds the tests share.

The squared distances are written component by component in the contract's order, so a contact decision here is the decision the
kernel takes.  The superpositions are tests/tm_ref.py's (csrc/horn.hpp operation by operation); every sum over atoms is a ``cumsum`` in
ascending (row, atom) order, and ``descending=True`` takes the atoms from the last one down instead: that changes the order of every
sum and nothing else, and the change of an output between the two orders is the yardstick of the GPU tests.
"""
from __future__ import annotations

import os

import numpy as np

import tm_ref as tr

MODES = ("ca", "cb", "backbone", "all")
CONTACT_CUTOFF = {"ca": 8.0, "cb": 8.0, "backbone": 5.0, "all": 5.0}
RECEPTOR, LIGAND = 1, 2
NO_NATIVE_CONTACT, TOO_FEW_ATOMS, DEGENERATE, EMPTY_SIDE, NOT_FINITE, SKIPPED = 1, 2, 4, 8, 16, 32
INT_OUTPUTS = ("n_native", "n_model", "n_shared", "n_interface_rows", "status")
ROW_OUTPUTS = ("res_native", "res_model", "res_shared", "interface_rows")
FLOAT_OUTPUTS = ("fnat", "fnonnat", "irmsd", "lrmsd", "dockq", "interface_rotation", "interface_translation", "receptor_rotation", "receptor_translation")
GAP_RULE = 1e-9        # the rotation is unique where top - second > GAP_RULE * scale (csrc/evaluate.hip)
COMPLEXES = ("1fyt", "5ksa", "7t2d")
MOTION_CASES = ("interleaved", "all64")  # the fixture holds them a second time with the model moved rigidly (<case>_moved)
# float32 rounding of the moved coordinates (|x| < 512: half an ulp is 2^-16 per axis) moves an atom by at most sqrt(3) 2^-16 A; the RMSD
# after the best superposition of a set of atoms changes by at most the root mean square of its atoms' displacements
MOTION_IRMSD = float(np.sqrt(3.0) * 2.0 ** -16)
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


def _layout(x):
    x = np.asarray(x)
    return x[:, None, :] if x.ndim == 2 else x


def set_columns(mode: str, layout: int):
    """The columns of the atom set in a layout of ``layout`` atoms per row (1: a CA trace); "cb": CA, CB."""
    if mode == "ca":
        return [0 if layout == 1 else 1]
    return [1, 3] if mode == "cb" else [0, 1, 2, 3, 4] if mode == "backbone" else list(range(37))


def rmsd_columns(mode: str, layout_a: int, layout_b: int):
    """(columns of the model, columns of the reference) of the RMSD atoms: N, CA, C, O, or CA alone."""
    if mode == "ca" or layout_a == 1 or layout_b == 1:
        return [0 if layout_a == 1 else 1], [0 if layout_b == 1 else 1]
    return [0, 1, 2, 4], [0, 1, 2, 4]


def exists(x, mask=None):
    """[N,A] bool: the project's convention (any non-zero coordinate) unless a mask is given."""
    return np.any(x != 0, axis=-1) if mask is None else np.asarray(mask).reshape(x.shape[:2]) != 0


def _sum_sq(dx, dy, dz):
    return (dx * dx + dy * dy) + dz * dz


def _cross_sq(x, y):
    """[len(x), len(y)] squared distances between the points x and y ([.,3] float64)."""
    return _sum_sq(x[:, None, 0] - y[None, :, 0], x[:, None, 1] - y[None, :, 1], x[:, None, 2] - y[None, :, 2])


def horn_gap(h):
    """(top - second, scale) of Horn's matrix of the covariance h [9]: the two numbers csrc/evaluate.hip's rule compares."""
    h = np.asarray(h, dtype=np.float64)
    a = np.array([[h[0] + h[4] + h[8], h[5] - h[7], h[6] - h[2], h[1] - h[3]], [h[5] - h[7], h[0] - h[4] - h[8], h[1] + h[3], h[6] + h[2]],
                  [h[6] - h[2], h[1] + h[3], h[4] - h[0] - h[8], h[5] + h[7]], [h[1] - h[3], h[6] + h[2], h[5] + h[7], h[8] - h[0] - h[4]]])
    if not np.all(np.isfinite(a)):
        return np.nan, np.nan
    w = np.linalg.eigvalsh(a)
    return float(w[3] - w[2]), float(np.abs(a).sum())


def _superpose(x, y, fit, evaluate, descending):
    """The device's superposition of the atoms ``fit`` of x onto y and the RMSD of the atoms ``evaluate`` under it.
    -> (rmsd, rotation [3,3], translation [3], status bits, relative eigenvalue gap or None)."""
    nan, zero = np.nan, (np.zeros((3, 3)), np.zeros(3))
    if fit.sum() < 3:
        return nan, *zero, TOO_FEW_ATOMS, None
    with np.errstate(all="ignore"):
        r, t = tr.superpose(fit[None], x, y, descending)
        m = float(fit.sum())
        c = [tr._ssum(np.where(fit, src[:, k], 0.0), descending) * (1.0 / m) for src in (x, y) for k in range(3)]
        h = [tr._ssum(np.where(fit, (x[:, i] - c[i]) * (y[:, j] - c[3 + j]), 0.0), descending) for i in range(3) for j in range(3)]
        gap, scale = horn_gap(h)
        status = 0 if gap > GAP_RULE * scale else DEGENERATE
        if evaluate.sum() == 0:
            return nan, r[0].reshape(3, 3), t[0], status | TOO_FEW_ATOMS, None
        d2 = tr.dist2(r, t, x, y)[0]
        rmsd = np.sqrt(tr._ssum(np.where(evaluate, d2, 0.0), descending) / float(evaluate.sum()))
    if not np.isfinite(rmsd):
        return nan, r[0].reshape(3, 3), t[0], status | NOT_FINITE, None
    return float(rmsd), r[0].reshape(3, 3), t[0], status, (gap / scale if scale > 0 else 0.0)


def interface_one(xa, xb, side, mode: str = "cb", mask_a=None, mask_b=None, res_mask_a=None, res_mask_b=None, contact_cutoff=None,
                  interface_cutoff: float = 10.0, descending: bool = False) -> dict:
    """xa (model), xb (reference): [N,37,3], [N,5,3] or [N,3] float32; side [N] in {0, 1, 2}.  Returns the device's outputs of the pair on
    this interface and, for the fixture, ``margin`` (the smallest |d^2 - c^2| / c^2 over every tested atom pair: the reference against
    both cutoffs, the model against the contact cutoff) and ``gaps`` (the relative eigenvalue gaps of the superpositions that ran)."""
    xa, xb, side = _layout(xa), _layout(xb), np.asarray(side).reshape(-1)
    n, la, lb = xa.shape[0], xa.shape[1], xb.shape[1]
    cc = CONTACT_CUTOFF[mode] if contact_cutoff is None else float(contact_cutoff)
    cc2, ic2 = cc * cc, float(interface_cutoff) * float(interface_cutoff)
    present = np.ones(n, dtype=bool)
    for m in (res_mask_a, res_mask_b):
        if m is not None:
            present &= np.asarray(m).reshape(-1) != 0
    ea, eb = exists(xa, mask_a), exists(xb, mask_b)
    ca_cols, cb_cols = set_columns(mode, la), set_columns(mode, lb)
    part = ea[:, ca_cols] & eb[:, cb_cols] & present[:, None]  # [N,K]
    if mode == "cb":
        part[:, 0] &= ~part[:, 1]
    pa, pb = xa[:, ca_cols].astype(np.float64), xb[:, cb_cols].astype(np.float64)
    receptor, ligand = present & (side == RECEPTOR), present & (side == LIGAND)
    out = {}
    ri, ru = np.nonzero(part & receptor[:, None])  # the receptor's atoms: row, atom of the set
    lj, lv = np.nonzero(part & ligand[:, None])
    d2b, d2a = _cross_sq(pb[ri, ru], pb[lj, lv]), _cross_sq(pa[ri, ru], pa[lj, lv])
    margin = np.inf
    for d2, c2 in ((d2b, cc2), (d2b, ic2), (d2a, cc2)):
        if d2.size:
            with np.errstate(invalid="ignore"):
                rel = np.abs(d2 - c2) / c2
            margin = min(margin, float(np.nanmin(rel))) if np.isfinite(rel).any() else margin

    def residue_pairs(close):
        i, j = np.nonzero(close)
        return np.unique(ri[i].astype(np.int64) * n + lj[j])

    native, model, near = residue_pairs(d2b <= cc2), residue_pairs(d2a <= cc2), residue_pairs(d2b <= ic2)
    shared = np.intersect1d(native, model)
    for key, codes in (("native", native), ("model", model), ("shared", shared)):
        out[f"n_{key}"] = len(codes)
        out[f"res_{key}"] = np.bincount(codes // n, minlength=n) + np.bincount(codes % n, minlength=n)
    rows = np.zeros(n, dtype=bool)
    rows[near // n] = rows[near % n] = True
    out["interface_rows"], out["n_interface_rows"] = rows, int(rows.sum())
    out["fnat"] = out["n_shared"] / out["n_native"] if out["n_native"] else 0.0
    out["fnonnat"] = (out["n_model"] - out["n_shared"]) / out["n_model"] if out["n_model"] else 0.0
    # the RMSD atoms, flattened in ascending (row, atom) order
    ra_cols, rb_cols = rmsd_columns(mode, la, lb)
    used = ea[:, ra_cols] & eb[:, rb_cols] & present[:, None]
    row, atom = np.nonzero(used)
    x, y = xa[:, ra_cols].astype(np.float64)[row, atom], xb[:, rb_cols].astype(np.float64)[row, atom]
    irmsd, ir, it, st_i, gap_i = _superpose(x, y, rows[row], rows[row], descending)
    lrmsd, lr, lt, st_l, gap_l = _superpose(x, y, receptor[row], ligand[row], descending)
    status = st_i | st_l | (0 if out["n_native"] else NO_NATIVE_CONTACT) | (0 if receptor.any() and ligand.any() else EMPTY_SIDE)
    if not out["n_native"]:
        irmsd = np.nan
    si, sl = irmsd / 1.5, lrmsd / 8.5
    out.update(irmsd=irmsd, lrmsd=lrmsd, dockq=(out["fnat"] + 1.0 / (1.0 + si * si) + 1.0 / (1.0 + sl * sl)) / 3.0, interface_rotation=ir,
               interface_translation=it, receptor_rotation=lr, receptor_translation=lt, status=status, margin=margin,
               gaps=[g for g in (gap_i, gap_l) if g is not None])
    return out


def interface_all(xa, xb, sides, mode="cb", **kw) -> dict:
    """``interface_one`` over the rows of ``sides`` [I,N], stacked: every output gains a leading axis I; ``margin`` is the smallest."""
    sides = np.atleast_2d(np.asarray(sides))
    each = [interface_one(xa, xb, s, mode, **kw) for s in sides]
    out = {k: np.stack([np.asarray(e[k]) for e in each]) for k in INT_OUTPUTS + ROW_OUTPUTS + FLOAT_OUTPUTS}
    out["margin"] = min(e["margin"] for e in each)
    out["gaps"] = [g for e in each for g in e["gaps"]]
    return out


def move(x, rot, shift):
    """The rigid motion of [..., 3] float32 coordinates, formed in float64 and rounded to float32; an absent atom (all zero) stays absent."""
    moved = (np.asarray(x, dtype=np.float64) @ np.asarray(rot).T + np.asarray(shift)).astype(np.float32)
    return np.where(np.any(np.asarray(x) != 0, axis=-1, keepdims=True), moved, np.float32(0))


def chain_contacts(pos, chain, cutoff=5.0):
    """An independent count for the tests of ``chain_sides``: pos [N,37,3] -> {(chain a, chain b), a < b: residue pairs with two atoms within
    ``cutoff``}, by a plain loop over the residues of the smaller chain against a distance matrix in float64."""
    pos = np.asarray(pos, dtype=np.float64)
    has = np.any(pos != 0, axis=-1)
    labels, counts = np.unique(chain), {}
    for i, a in enumerate(labels):
        for b in labels[i + 1:]:
            rows_a, rows_b = np.flatnonzero(chain == a), np.flatnonzero(chain == b)
            atoms_b = pos[rows_b][has[rows_b]]
            owner = np.repeat(np.arange(len(rows_b)), has[rows_b].sum(1))
            total = 0
            for r in rows_a:
                d = np.sqrt(((pos[r][has[r]][:, None, :] - atoms_b[None, :, :]) ** 2).sum(-1))
                total += len(np.unique(owner[(d <= cutoff).any(0)]))
            counts[(int(a), int(b))] = total
    return counts


# ---------------------------------------------------------------------------------------------- the fixture's cases
def complex_atom37(name: str):
    """(pos [N,37,3] float32, chain [N]) of one of the three complexes of tests/golden/sasa_cases.npz: the coordinates are read there by
    row and column, not copied."""
    z = np.load(os.path.join(GOLDEN, "sasa_cases.npz"))
    pos = np.zeros((len(z[f"{name}.aatype"]), 37, 3), dtype=np.float32)
    pos[z[f"{name}.row"].astype(np.int64), z[f"{name}.col"].astype(np.int64)] = z[f"{name}.xyz"]
    return pos, z[f"{name}.chain"].astype(np.int64)


def noisy_chain(pos, chain, label: int, seed: int, sigma: float = 1.0):
    """pos with N(0, sigma) added to every existing atom of chain ``label`` (the frozen stream of ``RandomState``), float32."""
    rng = np.random.RandomState(seed)
    noise = rng.normal(0.0, sigma, size=pos.shape).astype(np.float32)
    rows = (np.asarray(chain) == label)[:, None, None] & np.any(pos != 0, axis=-1, keepdims=True)
    return np.where(rows, pos + noise, pos).astype(np.float32)


def loop_window(chain, label: int, start: int, length: int = 12):
    """[N] bool: rows start .. start + length - 1 of chain ``label`` (counted inside the chain)."""
    rows = np.flatnonzero(np.asarray(chain) == label)[start:start + length]
    mask = np.zeros(len(chain), dtype=bool)
    mask[rows] = True
    return mask


def bound(fix, case: str, key: str, value) -> float:
    """32 x the restatement's own change between its two summation orders; where that is 0, 32 ulp of the value."""
    yard = float(fix[f"{case}.{key}.yard"])
    if yard > 0:
        return 32.0 * yard
    value = np.abs(np.asarray(value, dtype=np.float64)).reshape(-1)
    return 32.0 * float(np.max(np.spacing(value))) if value.size and np.all(np.isfinite(value)) else 0.0


def case_inputs(fix, name: str):
    """(model [N,A,3], reference [N,A_b,3], sides [I,N] int32, mode) of a recorded case; a real complex is rebuilt from the SASA fixture and
    the recorded noise seed."""
    mode, sides = str(fix[f"{name}.mode"]), fix[f"{name}.sides"].astype(np.int32)
    if f"{name}.xa" in fix:
        return fix[f"{name}.xa"], fix[f"{name}.xb"], sides, mode
    pos, chain = complex_atom37(name.split(".")[0])
    return noisy_chain(pos, chain, int(fix[f"{name}.label"]), int(fix[f"{name}.seed"])), pos, sides, mode


def check_case(fix, name: str, got: dict, p: int = 0, report=None):
    """Pair ``p`` of a device result against the recorded restatement of ``name``: integers, masks and status exactly; the float outputs
    (where the case compares them) NaN where the restatement is and within ``bound`` elsewhere.  ``report(key, error, bound)``."""
    for k in INT_OUTPUTS + ROW_OUTPUTS:
        assert np.array_equal(np.asarray(got[k])[p], fix[f"{name}.{k}"]), (name, k)
    if not int(fix[f"{name}.floats"]):
        return
    for k in FLOAT_OUTPUTS:
        want, have = fix[f"{name}.{k}"], np.asarray(got[k])[p]
        assert have.dtype == np.float64 and np.array_equal(np.isnan(want), np.isnan(have)), (name, k)
        err, lim = float(np.max(np.abs(have - want)[~np.isnan(want)], initial=0.0)), bound(fix, name, k, want[~np.isnan(want)])
        if report is not None:
            report(k, err, lim)
        assert err <= lim, (name, k, err, lim)
