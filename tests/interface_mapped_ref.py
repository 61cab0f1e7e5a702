"""NumPy restatement of the mapped interface-accuracy contract (include/fdipt.h "interface accuracy through a row map", DESIGN.md section
7.19) in both coverage modes, written directly: own loops over the reference's existing and covered rows, with tests/interface_ref.py's
``_superpose`` and ``_sum_sq`` for the arithmetic.  Also the builders of the two oracle models - the gathered model (coverage "ignore")
and the far-point model (coverage "penalise") - and the cases the host tests, the GPU tests and the fixture
tests/golden/interface_mapped_cases.npz (tests/golden/make_goldens_interface_mapped.py) share: they are cut from the complexes
``interface_ref.complex_atom37`` serves, so the fixture records results and yardsticks only.
"""
from __future__ import annotations

import functools

import numpy as np

import interface_ref as ir

COUNT_OUTPUTS = ("n_native", "n_model", "n_shared", "n_interface_rows")  # what the far-point oracle pins, with ROW_OUTPUTS
INT_OUTPUTS = ir.INT_OUTPUTS + ("n_interface_covered",)
MAP_OUT_OF_RANGE, MAP_DUPLICATE = 64, 128  # FDIPT_IFACE_MAP_OUT_OF_RANGE, FDIPT_IFACE_MAP_DUPLICATE
FAR = 1.0e5  # A: where the far-point model puts the first atom of reference row 0; rows are 1000 A apart, atoms of a row 20 A


def resolve(m, res_mask_a, res_mask_b, n_a: int):
    """(mrow [N_b] int64: the model row of every covered reference row, -1 elsewhere; exists [N_b] bool)."""
    m = np.asarray(m, dtype=np.int64).reshape(-1)
    exists = np.ones(len(m), dtype=bool) if res_mask_b is None else np.asarray(res_mask_b).reshape(-1) != 0
    rows_a = np.ones(n_a, dtype=bool) if res_mask_a is None else np.asarray(res_mask_a).reshape(-1) != 0
    mrow = np.full(len(m), -1, dtype=np.int64)
    for j in range(len(m)):
        if exists[j] and 0 <= m[j] < n_a and rows_a[m[j]]:
            mrow[j] = m[j]
    return mrow, exists


def mapped_one(xa, xb, side, m, mode: str = "cb", coverage: str = "ignore", mask_a=None, mask_b=None, res_mask_a=None, res_mask_b=None,
               contact_cutoff=None, interface_cutoff: float = 10.0, descending: bool = False) -> dict:
    """xa [N_a,...] (model), xb [N_b,...] (reference), side [N_b], m [N_b]: the outputs of one pair on one interface, plus ``n_covered``
    and ``n_reference`` and, for the fixture, ``gaps`` (the relative eigenvalue gaps of the superpositions that ran)."""
    xa, xb, side = ir._layout(xa), ir._layout(xb), np.asarray(side).reshape(-1)
    n_a, n_b, la, lb = xa.shape[0], xb.shape[0], xa.shape[1], xb.shape[1]
    cc = ir.CONTACT_CUTOFF[mode] if contact_cutoff is None else float(contact_cutoff)
    cc2, ic2 = cc * cc, float(interface_cutoff) * float(interface_cutoff)
    mrow, exists = resolve(m, res_mask_a, res_mask_b, n_a)
    covered = mrow >= 0
    takes = covered if coverage == "ignore" else exists
    ea, eb = ir.exists(xa, mask_a), ir.exists(xb, mask_b)
    cols_a, cols_b = ir.set_columns(mode, la), ir.set_columns(mode, lb)
    k_set = len(cols_b)
    part = np.zeros((n_b, k_set), dtype=bool)  # the atoms of the set that take part, per reference row
    for j in np.flatnonzero(takes):
        for k in range(k_set):
            part[j, k] = eb[j, cols_b[k]] and (ea[mrow[j], cols_a[k]] if covered[j] else True)
        if mode == "cb" and part[j, 1]:
            part[j, 0] = False
    pb = xb[:, cols_b].astype(np.float64)
    pa = np.zeros((n_b, k_set, 3))  # the model in reference rows (zeros where there is none: never read)
    pa[covered] = xa[mrow[covered]][:, cols_a].astype(np.float64)
    receptor, ligand = takes & (side == ir.RECEPTOR), takes & (side == ir.LIGAND)
    lig_row, lig_atom = np.nonzero(part & ligand[:, None])
    yb, ya, lig_cov = pb[lig_row, lig_atom], pa[lig_row, lig_atom], covered[lig_row]
    res = {k: np.zeros(n_b, dtype=np.int64) for k in ("native", "model", "shared")}
    rows = np.zeros(n_b, dtype=bool)
    for i in np.flatnonzero(receptor):
        nat, mod, near = np.zeros(n_b, dtype=bool), np.zeros(n_b, dtype=bool), np.zeros(n_b, dtype=bool)
        for u in np.flatnonzero(part[i]):
            d2b = ir._sum_sq(pb[i, u, 0] - yb[:, 0], pb[i, u, 1] - yb[:, 1], pb[i, u, 2] - yb[:, 2])
            nat[lig_row[d2b <= cc2]] = True
            near[lig_row[d2b <= ic2]] = True
            if covered[i]:  # a contact of the model needs both rows in the model
                d2a = ir._sum_sq(pa[i, u, 0] - ya[:, 0], pa[i, u, 1] - ya[:, 1], pa[i, u, 2] - ya[:, 2])
                mod[lig_row[(d2a <= cc2) & lig_cov]] = True
        for key, hit in (("native", nat), ("model", mod), ("shared", nat & mod)):
            res[key][i] += int(hit.sum())
            res[key] += hit
        if near.any():
            rows[i] = True
            rows |= near
    out = {f"res_{k}": v for k, v in res.items()}
    out.update({f"n_{k}": int(v[receptor].sum()) for k, v in res.items()})
    out["interface_rows"], out["n_interface_rows"], out["n_interface_covered"] = rows, int(rows.sum()), int((rows & covered).sum())
    out["fnat"] = out["n_shared"] / out["n_native"] if out["n_native"] else 0.0
    out["fnonnat"] = (out["n_model"] - out["n_shared"]) / out["n_model"] if out["n_model"] else 0.0
    # the RMSD atoms: covered rows only, flattened in ascending (reference row, atom) order
    ra_cols, rb_cols = ir.rmsd_columns(mode, la, lb)
    row, atom = [], []
    for j in np.flatnonzero(covered & takes):
        for r in range(len(ra_cols)):
            if ea[mrow[j], ra_cols[r]] and eb[j, rb_cols[r]]:
                row.append(j)
                atom.append(r)
    row, atom = np.asarray(row, dtype=np.int64), np.asarray(atom, dtype=np.int64)
    x = xa[mrow[row]][np.arange(len(row)), np.asarray(ra_cols)[atom]].astype(np.float64).reshape(-1, 3)
    y = xb[row, np.asarray(rb_cols)[atom]].astype(np.float64).reshape(-1, 3)
    irmsd, i_rot, i_t, st_i, gap_i = ir._superpose(x, y, rows[row], rows[row], descending)
    lrmsd, l_rot, l_t, st_l, gap_l = ir._superpose(x, y, receptor[row], ligand[row], descending)
    status = st_i | st_l | (0 if out["n_native"] else ir.NO_NATIVE_CONTACT) | (0 if receptor.any() and ligand.any() else ir.EMPTY_SIDE)
    if not out["n_native"]:
        irmsd = np.nan
    si, sl = irmsd / 1.5, lrmsd / 8.5
    out.update(irmsd=irmsd, lrmsd=lrmsd, dockq=(out["fnat"] + 1.0 / (1.0 + si * si) + 1.0 / (1.0 + sl * sl)) / 3.0, interface_rotation=i_rot,
               interface_translation=i_t, receptor_rotation=l_rot, receptor_translation=l_t, status=status, n_covered=int(covered.sum()),
               n_reference=int(exists.sum()), gaps=[g for g in (gap_i, gap_l) if g is not None])
    return out


def mapped_all(xa, xb, sides, m, mode="cb", coverage="ignore", **kw) -> dict:
    """``mapped_one`` over the rows of ``sides`` [I,N_b], stacked."""
    each = [mapped_one(xa, xb, s, m, mode, coverage, **kw) for s in np.atleast_2d(np.asarray(sides))]
    out = {k: np.stack([np.asarray(e[k]) for e in each]) for k in INT_OUTPUTS + ir.ROW_OUTPUTS + ir.FLOAT_OUTPUTS}
    out.update(n_covered=each[0]["n_covered"], n_reference=each[0]["n_reference"], gaps=[g for e in each for g in e["gaps"]])
    return out


# ---------------------------------------------------------------------------------------------- the two oracle models
def _pattern(eb, la: int, lb: int):
    """The reference's atom pattern [N_b,lb] in the columns of a model layout of ``la`` atoms per row."""
    if la == lb:
        return eb.copy()
    out = np.zeros((len(eb), la), dtype=bool)
    if la == 1:
        out[:, 0] = eb[:, 1]
    elif lb == 1:
        out[:, 1] = eb[:, 0]
    else:
        out[:, :min(la, lb)] = eb[:, :min(la, lb)]
    return out


def gathered_model(xa, m, res_mask_a=None, mask_a=None, res_mask_b=None):
    """(model [N_b,...], res_mask [N_b] float32, atom mask or None) in reference rows: row j is model row m[j] where covered and is
    masked off by res_mask elsewhere.  The oracle of coverage "ignore": the un-mapped entry on it gives every output."""
    xa = np.asarray(xa)
    mrow, _ = resolve(m, res_mask_a, res_mask_b, len(xa))
    out, keep = np.zeros((len(mrow),) + xa.shape[1:], dtype=xa.dtype), mrow >= 0
    out[keep] = xa[mrow[keep]]
    mask = None
    if mask_a is not None:
        mask = np.zeros((len(mrow),) + np.asarray(mask_a).shape[1:], dtype=np.asarray(mask_a).dtype)
        mask[keep] = np.asarray(mask_a)[mrow[keep]]
    return out, keep.astype(np.float32), mask


def far_point_model(xa, xb, m, res_mask_a=None, mask_a=None, res_mask_b=None, mask_b=None):
    """(model [N_b,...], res_mask [N_b] float32, atom mask [N_b,la] uint8): the gathered model with every uncovered EXISTING reference row
    given the reference row's atom pattern at a far, distinct point - row j, atom u at (FAR + 1000 j, 20 u, 0): beyond both cutoffs from
    every atom and from each other -, marked present.  The oracle of coverage "penalise" for the counts and the per-row outputs."""
    xa3, xb3 = ir._layout(np.asarray(xa)), ir._layout(np.asarray(xb))
    la, lb = xa3.shape[1], xb3.shape[1]
    mrow, exists = resolve(m, res_mask_a, res_mask_b, len(xa3))
    out, mask = np.zeros((len(mrow), la, 3), dtype=np.float32), np.zeros((len(mrow), la), dtype=np.uint8)
    keep = mrow >= 0
    out[keep], mask[keep] = xa3[mrow[keep]], ir.exists(xa3, mask_a)[mrow[keep]]
    pattern = _pattern(ir.exists(xb3, mask_b), la, lb)
    for j in np.flatnonzero(exists & ~keep):
        for u in np.flatnonzero(pattern[j]):
            out[j, u], mask[j, u] = (FAR + 1000.0 * j, 20.0 * u, 0.0), 1
    if np.asarray(xa).ndim == 2:
        out, mask = out[:, 0], mask[:, 0]
    return out, exists.astype(np.float32), mask


# ---------------------------------------------------------------------------------------------- the shared cases
def cut_complex(name: str, receptor: int, ligand: int, n_rec: int, n_lig: int, ligand_first: bool = False):
    """(pos [n_rec + n_lig,37,3], sides [1,N], chain [N], aatype [N]): the ``n_rec`` rows of chain ``receptor`` and the ``n_lig`` rows of
    chain ``ligand`` whose CA is nearest to a CA of the other chain, each chain in its own row order."""
    pos, chain = ir.complex_atom37(name)
    aatype = np.load(ir.os.path.join(ir.GOLDEN, "sasa_cases.npz"))[f"{name}.aatype"].astype(np.int64)
    ca = pos[:, 1].astype(np.float64)
    rows_r, rows_l = np.flatnonzero(chain == receptor), np.flatnonzero(chain == ligand)
    d = np.sqrt(((ca[rows_r][:, None] - ca[rows_l][None]) ** 2).sum(-1))
    keep_r = np.sort(rows_r[np.argsort(d.min(1), kind="stable")[:n_rec]])
    keep_l = np.sort(rows_l[np.argsort(d.min(0), kind="stable")[:n_lig]])
    assert len(keep_r) == n_rec and len(keep_l) == n_lig
    rows = np.concatenate([keep_l, keep_r] if ligand_first else [keep_r, keep_l])
    sides = np.where(chain[rows] == receptor, ir.RECEPTOR, ir.LIGAND).astype(np.int32)[None]
    return pos[rows], sides, chain[rows], aatype[rows]


def plant(xb_noisy, src, filler):
    """The model [N_a,...] whose row r holds row src[r] of ``xb_noisy`` (the model in reference rows), or, where src[r] < 0, an inserted
    row nothing maps to, taken from ``filler``; and the map [N_b] that finds the rows again."""
    src = np.asarray(src, dtype=np.int64)
    xa = np.where((src >= 0).reshape((-1,) + (1,) * (xb_noisy.ndim - 1)), xb_noisy[np.maximum(src, 0)], filler[:len(src)]).astype(np.float32)
    m = np.full(len(xb_noisy), -1, dtype=np.int32)
    m[src[src >= 0]] = np.flatnonzero(src >= 0)
    return xa, m


def _window(n_b, lo, hi):
    return np.array([j for j in range(n_b) if not lo <= j <= hi], dtype=np.int64)


@functools.lru_cache(maxsize=None)
def cases() -> dict:
    """name -> dict(xa [N_a,...], xb [N_b,...], sides [I,N_b], mode, m [N_b], res_mask_a [N_a] or None): sizes at the kernel's edges (64
    receptor rows per block; ligand tiles of 256 rows, 64 for "all") and maps that leave whole blocks and tiles without a model row."""
    out = {}

    def add(name, mode, xb, sides, src, model_atoms=37, res_mask_a=None, seed=7):
        noisy = ir.noisy_chain(xb, sides[0], ir.LIGAND, seed, 1.0)  # (1 A on the ligand: 0 < fnat < 1)
        filler = (ir.noisy_chain(xb, sides[0], ir.RECEPTOR, seed + 1, 3.0) + np.float32(40.0) * (xb != 0))[::-1]  # inserted rows: 40 A away
        filler = np.concatenate([filler] * (1 + len(src) // len(filler)))
        xa, m = plant(noisy, src, filler)
        if model_atoms == 5:
            xa = xa[:, :5]
        elif model_atoms == 1:
            xa, xb = xa[:, 1], xb[:, 1]
        out[name] = dict(xa=np.ascontiguousarray(xa), xb=np.ascontiguousarray(xb), sides=sides, mode=mode, m=m, res_mask_a=res_mask_a)

    # N_b = 65 (ligand rows 0 .. 29, receptor rows 30 .. 64: row 64 is the only row of the second block), N_a = 70
    xb, sides, _, _ = cut_complex("1fyt", 0, 1, 35, 30, ligand_first=True)
    ident = np.arange(65)
    add("n65.insert", "cb", xb, sides, np.concatenate([ident[:20], [-1] * 5, ident[20:]]))  # every row covered, 5 inserted model rows
    add("n65.window", "cb", xb, sides, np.concatenate([_window(65, 62, 64), [-1] * 8]))  # rows 62 .. 64 deleted: the second block has no model row
    mask = np.ones(70, dtype=np.float32)
    mask[[3, 40]] = 0  # model rows 3 (a ligand row) and 40 (a receptor row) are dropped by res_mask
    add("n65.masked", "ca", xb, sides, np.concatenate([ident, [-1] * 5]), res_mask_a=mask)
    add("n65.backbone", "backbone", xb, sides, np.concatenate([_window(65, 10, 14), [-1] * 10]))
    # N_b = 257 (receptor rows 0 .. 139, ligand rows 140 .. 256: row 256 is the only row of the second ligand tile), N_a = 200 < N_b;
    # an atom37 reference against a five-atom model
    xb, sides, _, _ = cut_complex("5ksa", 3, 2, 140, 117)
    add("n257.window", "backbone", xb, sides, np.concatenate([_window(257, 200, 256)[:196], [-1] * 4]), model_atoms=5)  # rows 196 .. 256 open
    add("n257.tile", "cb", xb, sides, np.concatenate([np.arange(60, 255)[::-1], [-1] * 4, [256]]), model_atoms=5)  # rows 0 .. 59 and 255 open, reversed
    # N_b = 130 for "all" (receptor rows 0 .. 69, ligand rows 70 .. 129: ligand tiles of 64 rows)
    xb, sides, _, _ = cut_complex("7t2d", 0, 1, 70, 60)
    add("all130.swapped", "all", xb, sides, np.concatenate([np.arange(70, 130), np.arange(70)]))  # the model stores the ligand chain first
    add("all130.tile", "all", xb, sides, np.concatenate([np.arange(70), np.arange(128, 130)]))  # no ligand row of tile 64 .. 127 has a model row
    add("all130.window", "all", xb, sides, _window(130, 60, 75))
    # the smallest: one row per side, CA traces
    xb, sides, _, _ = cut_complex("1fyt", 0, 1, 1, 1)
    add("n2.swapped", "ca", xb, sides, np.array([1, 0]), model_atoms=1)
    add("n2.open", "ca", xb, sides, np.array([0, -1]), model_atoms=1)
    return out


def case_kw(case: dict) -> dict:
    """The keyword arguments of ``mapped_all`` for a case."""
    return dict(mode=case["mode"], res_mask_a=case["res_mask_a"])
