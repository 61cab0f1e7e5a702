"""NumPy restatement of the secondary-structure contract (include/fdipt.h, "secondary structure"): Kabsch &
Sander's hydrogen-bond patterns in the simplified alphabet C / H / E, written from the contract's text with whole-matrix operations -
the kernel (csrc/dssp.hip) walks candidate pairs instead - so that the two share the rules and nothing else.  float64 throughout.

``dssp(bb, ...)`` takes ONE sample: bb [N,4,3] float32 (N, CA, C, O) or [N,37,3] / [N,5,3] (atom37 columns 0, 1, 2, 4).
"""
from __future__ import annotations

import numpy as np

COIL, HELIX, STRAND, ABSENT = 0, 1, 2, 255
LETTERS = {COIL: "C", HELIX: "H", STRAND: "E"}
PARALLEL, ANTIPARALLEL = 1, 2
Q = -27.888          # kcal/mol: 332 * 0.42 * 0.20
E_MIN = -9.9
E_BOND = -0.5
CA_CUTOFF = 9.0
BREAK_CN = 2.5
D_MIN = 0.5
SLOTS_PER_ROW = 8    # bridges (i, .) a row i can form under the two-slot limit
INTEGER_OUTPUTS = ("ss", "n_rows", "n_hbonds", "n_bridges", "n_ladders", "acceptor", "status")
FRACTIONS = ("helix_percent", "strand_percent", "coil_percent", "non_coil_percent")


def backbone4(x):
    """[..., 4, 3] (N, CA, C, O) of an atom37 / five-atom / four-atom array."""
    x = np.asarray(x)
    return x if x.shape[-2] == 4 else x[..., [0, 1, 2, 4], :]


def round_half_away(v):
    """C ``round``: to the nearest integer, halves away from zero (``np.round`` rounds halves to even)."""
    v = np.asarray(v, dtype=np.float64)
    return np.sign(v) * np.floor(np.abs(v) + 0.5)


def round_energy(raw):
    """An energy as the slots keep it: three decimals, halves away from zero, not below -9.9."""
    return np.maximum(round_half_away(np.asarray(raw, dtype=np.float64) * 1000.0) / 1000.0, E_MIN)


def existing_rows(bb, res_mask=None):
    bb = backbone4(bb)
    exists = np.any(bb != 0, axis=-1).all(axis=-1)
    if res_mask is not None:
        exists &= np.asarray(res_mask) != 0
    return np.flatnonzero(exists)


def _dist(a, b):
    d = a - b
    return np.sqrt(d[..., 0] * d[..., 0] + d[..., 1] * d[..., 1] + d[..., 2] * d[..., 2])


def hbond_energies(x, brk, proline):
    """x [n,4,3] float64, brk [n] bool, proline [n] bool -> (raw [n,n] energies before rounding, final [n,n] rounded and clamped,
    valid [n,n]: the pairs (donor, acceptor) the contract evaluates)."""
    n = len(x)
    nn, ca, c, o = x[:, 0], x[:, 1], x[:, 2], x[:, 3]
    h = nn.copy()
    for k in range(1, n):
        if not brk[k]:
            co = c[k - 1] - o[k - 1]
            h[k] = nn[k] + co / np.sqrt(co[0] * co[0] + co[1] * co[1] + co[2] * co[2])
    d_ho, d_hc = _dist(h[:, None], o[None]), _dist(h[:, None], c[None])
    d_nc, d_no = _dist(nn[:, None], c[None]), _dist(nn[:, None], o[None])
    idx = np.arange(n)
    valid = (idx[:, None] != idx[None]) & (idx[None] != idx[:, None] - 1) & (_dist(ca[:, None], ca[None]) < CA_CUTOFF) & ~proline[:, None]
    with np.errstate(divide="ignore", invalid="ignore"):
        raw = Q * (((1.0 / d_ho - 1.0 / d_hc) + 1.0 / d_nc) - 1.0 / d_no)
    close = np.minimum(np.minimum(d_ho, d_hc), np.minimum(d_nc, d_no)) < D_MIN
    final = np.where(close, E_MIN, round_energy(np.where(close, 0.0, raw)))
    return np.where(valid, raw, 0.0), np.where(valid, final, 0.0), valid, close


def two_slots(final):
    """Per donor its two best acceptors: lowest energy, lower index on equal energy, energies below 0 only.  -> acc [n,2] (-1: none),
    en [n,2] (0: none)."""
    n = len(final)
    acc, en = np.full((n, 2), -1, dtype=np.int64), np.zeros((n, 2))
    e = final.copy()
    for s in range(2):
        if n == 0:
            break
        best = np.argmin(e, axis=1)  # (the first of equal minima: the lower index)
        val = e[np.arange(n), best]
        ok = val < 0
        acc[ok, s], en[ok, s] = best[ok], val[ok]
        e[np.arange(n), best] = np.inf
    return acc, en


def dssp(bb, res_mask=None, chain_idx=None, is_proline=None, bulges=True):
    """One sample.  Returns the outputs of ``fdipt_sample_dssp`` for it (INTEGER_OUTPUTS, FRACTIONS, ``acceptor_energy``) and, for the
    fixture's yardsticks, ``raw_energy`` [n,n] / ``valid`` / ``rows`` / ``ladders`` (type, ib, ie, jb, je after merging) /
    ``half_margin`` (the smallest distance of 1000 E from a half-integer over the evaluated pairs)."""
    bb = backbone4(bb)
    big_n = bb.shape[0]
    rows = existing_rows(bb, res_mask)
    n = len(rows)
    x = bb[rows].astype(np.float64)
    chain = np.zeros(big_n, dtype=np.int64) if chain_idx is None else np.asarray(chain_idx).astype(np.int64)
    chain = chain[rows]
    proline = (np.zeros(big_n, dtype=bool) if is_proline is None else np.asarray(is_proline) != 0)[rows]

    brk = np.ones(n, dtype=bool)
    for k in range(1, n):
        brk[k] = chain[k] != chain[k - 1] or _dist(x[k - 1, 2], x[k, 0]) > BREAK_CN
    before = np.concatenate([[0], np.cumsum(brk)])  # before[k]: breaks before rows < k

    def no_break(a, b):
        """Rows a..b follow each other: none of the rows a + 1 .. b has a break before it."""
        return before[b + 1] - before[a + 1] == 0

    raw, final, valid, close = hbond_energies(x, brk, proline)
    acc, en = two_slots(final)
    hb = np.zeros((n, n), dtype=bool)
    for s in range(2):
        d = np.flatnonzero((acc[:, s] >= 0) & (en[:, s] < E_BOND))
        hb[d, acc[d, s]] = True

    turn = {m: np.array([i + m < n and hb[i + m, i] and no_break(i, i + m) for i in range(n)], dtype=bool) for m in (3, 4, 5)}

    kind = np.zeros((n, n), dtype=np.int8)
    if n >= 3:  # rows 1 .. n - 2 as i and as j: [i - 1, j - 1] of the inner arrays below is the pair (i, j)
        inner = np.arange(1, n - 1)
        whole = np.array([no_break(k - 1, k + 1) for k in inner], dtype=bool)
        up, mid = hb[2:], hb[1:-1]  # donor i + 1, i
        para = (up[:, 1:-1] & mid[:, :-2].T) | (up[:, 1:-1].T & mid[:, :-2])
        anti = (up[:, :-2] & up[:, :-2].T) | (mid[:, 1:-1].T & mid[:, 1:-1])
        allowed = whole[:, None] & whole[None] & (inner[None] >= inner[:, None] + 3)
        kind[1:-1, 1:-1] = np.where(allowed & para, PARALLEL, np.where(allowed & anti, ANTIPARALLEL, 0))

    ladders = []  # [type, ib, ie, jb, je]
    for i, j in zip(*np.nonzero(kind)):
        t = kind[i, j]
        step = 1 if t == PARALLEL else -1
        if 0 <= j - step < n and kind[i - 1, j - step] == t:
            continue  # not the first bridge of its run
        k = 0
        while i + k + 1 < n and 0 <= j + step * (k + 1) < n and kind[i + k + 1, j + step * (k + 1)] == t:
            k += 1
        ladders.append([int(t), int(i), int(i + k), int(min(j, j + step * k)), int(max(j, j + step * k))])
    n_bridges = int(np.count_nonzero(kind))
    ladders.sort(key=lambda l: (l[1], l[3], l[0], l[4]))
    if bulges:
        a = 0
        while a < len(ladders):
            b = a + 1
            while b < len(ladders):
                ta, iba, iea, jba, jea = ladders[a]
                tb, ibb, ieb, jbb, jeb = ladders[b]
                gap_i = ibb - iea
                g = jbb - jea if ta == PARALLEL else jba - jeb
                if (ta == tb and no_break(min(iba, ibb), max(iea, ieb)) and no_break(min(jba, jbb), max(jea, jeb)) and 0 < gap_i < 6 and g > 0
                        and ((g < 6 and gap_i < 3) or g < 3)):
                    ladders[a] = [ta, iba, ieb, min(jba, jbb), max(jea, jeb)]
                    del ladders[b]
                else:
                    b += 1
            a += 1

    state = np.zeros(n, dtype=np.int8)  # 0 none, 2 E, 3 alpha, 4 3-10, 5 pi
    for _, ib, ie, jb, je in ladders:
        state[ib:ie + 1] = 2
        state[jb:je + 1] = 2
    for i in range(1, n):
        if turn[4][i - 1] and turn[4][i]:
            state[i:i + 4] = 3
    for code, m in ((4, 3), (5, 5)):
        prev = state.copy()
        for i in range(1, n):
            if turn[m][i - 1] and turn[m][i] and (prev[i:i + m] == 0).all():
                state[i:i + m] = code
    cls = np.where(state == 2, STRAND, np.where(state >= 3, HELIX, COIL)).astype(np.uint8)

    ss = np.full(big_n, ABSENT, dtype=np.uint8)
    ss[rows] = cls
    acceptor = np.full((big_n, 2), -1, dtype=np.int32)
    energy = np.zeros((big_n, 2))
    acceptor[rows] = np.where(acc >= 0, rows[np.maximum(acc, 0)] if n else acc, -1)
    energy[rows] = en
    counts = [int((cls == c).sum()) for c in (HELIX, STRAND, COIL)]
    frac = [c / n if n else np.nan for c in counts]
    evaluated = raw[valid & ~close] * 1000.0
    margin = float(np.min(np.abs(np.abs(evaluated - np.floor(evaluated)) - 0.5), initial=np.inf))
    return {"ss": ss, "n_rows": n, "n_hbonds": int(hb.sum()), "n_bridges": n_bridges, "n_ladders": len(ladders), "acceptor": acceptor,
            "acceptor_energy": energy, "status": 0, "helix_percent": frac[0], "strand_percent": frac[1], "coil_percent": frac[2],
            "non_coil_percent": (counts[0] + counts[1]) / n if n else np.nan,
            "bridges_per_row": np.count_nonzero(kind, axis=1), "raw_energy": raw, "valid": valid, "rows": rows, "ladders": ladders, "half_margin": margin, "turns": turn, "hb": hb}


def ss_string(ss):
    return "".join(LETTERS[int(c)] for c in np.asarray(ss) if c != ABSENT)


def place(a, b, c, bond, angle, torsion):
    """The point at ``bond`` from c with the angle b-c-d and the dihedral a-b-c-d (degrees)."""
    angle, torsion = np.deg2rad(angle), np.deg2rad(torsion)
    bc = (c - b) / np.linalg.norm(c - b)
    nrm = np.cross(b - a, bc)
    nrm /= np.linalg.norm(nrm)
    frame = np.stack([bc, np.cross(nrm, bc), nrm], axis=1)
    return c + frame @ (bond * np.array([-np.cos(angle), np.sin(angle) * np.cos(torsion), np.sin(angle) * np.sin(torsion)]))


def ideal_backbone(n, phi, psi, origin=(12.0, -7.0, 30.0)):
    """[n,4,3] float32 (N, CA, C, O) from constant phi / psi: bonds C-N 1.329, N-CA 1.458, CA-C 1.525, C=O 1.231, angles CA-C-N 116.2,
    C-N-CA 121.7, N-CA-C 111.0, CA-C-O 120.5, omega 180; away from the origin so that no atom has three zero coordinates."""
    x = np.zeros((n, 4, 3))
    x[0, 0], x[0, 1] = [0.0, 0.0, 0.0], [1.458, 0.0, 0.0]
    x[0, 2] = x[0, 1] + 1.525 * np.array([-np.cos(np.deg2rad(111.0)), np.sin(np.deg2rad(111.0)), 0.0])
    for i in range(n):
        if i > 0:
            x[i, 0] = place(x[i - 1, 0], x[i - 1, 1], x[i - 1, 2], 1.329, 116.2, psi)
            x[i, 1] = place(x[i - 1, 1], x[i - 1, 2], x[i, 0], 1.458, 121.7, 180.0)
            x[i, 2] = place(x[i - 1, 2], x[i, 0], x[i, 1], 1.525, 111.0, phi)
        x[i, 3] = place(x[i, 0], x[i, 1], x[i, 2], 1.231, 120.5, psi + 180.0)
    return (x + np.asarray(origin)).astype(np.float32)


# name: (phi, psi, the classes of a 20-residue chain)
IDEAL = {"alpha": (-57.0, -47.0, "C" + "H" * 18 + "C"), "three_ten": (-49.0, -26.0, "C" + "H" * 18 + "C"),
         "pi": (-57.0, -70.0, "C" + "H" * 18 + "C"), "extended": (-120.0, 130.0, "C" * 20), "ppii": (-75.0, 145.0, "C" * 20)}

# the cases of tests/golden/dssp_cases.npz (make_goldens_dssp.py): the three complexes, then the excerpts
COMPLEXES = ("1fyt", "5ksa", "7t2d")


def case_names(fix):
    return [str(s) for s in fix["cases"]]


def case_inputs(fix, name):
    """One fixture case as the arguments of ``dssp``."""
    return {"bb": fix[f"{name}.bb"], "chain_idx": fix[f"{name}.chain_idx"], "is_proline": fix[f"{name}.is_proline"]}


def three_acceptor_case():
    """Five rows: a donor (row 1, with row 0 before it in its chain, so that its H is one Angstrom along +x from its N) and three
    carbonyls of three other chains that point at the H from three sides at 2.0, 2.1 and 2.2 Angstrom: three energies below -0.5, of
    which the two slots keep the first two.  -> bb [5,4,3] float32, chain_idx [5]."""
    shift = np.array([10.0, 10.0, 10.0])
    bb = np.zeros((5, 4, 3))
    bb[0] = [[-2.9, -2.6, 0.3], [-1.9, -1.7, 0.2], [-0.6, -1.2, 0.0], [-1.83, -1.2, 0.0]]   # C - O along +x, C 1.34 from the donor's N
    bb[1] = [[0.0, 0.0, 0.0], [-0.5, 1.3, 0.3], [-1.9, 1.6, 0.9], [-2.3, 2.7, 1.2]]
    for k, (phi, reach) in enumerate(((0.0, 2.0), (120.0, 2.1), (240.0, 2.2))):
        u = np.array([0.5, np.sqrt(0.75) * np.cos(np.deg2rad(phi)), np.sqrt(0.75) * np.sin(np.deg2rad(phi))])
        o = np.array([1.0, 0.0, 0.0]) + reach * u
        c = o + 1.231 * u
        ca = c + 1.525 * (u + np.array([0.3, 0.0, 0.0])) / np.linalg.norm(u + np.array([0.3, 0.0, 0.0]))
        bb[2 + k] = [ca + 1.458 * u, ca, c, o]
    return (bb + shift).astype(np.float32), np.array([0, 0, 1, 2, 3], dtype=np.int32)
