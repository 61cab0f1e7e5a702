"""Deterministic edge cases for the IPA attention kernels (csrc/attention.hip, csrc/attention3.hip) — test infrastructure.

NumPy only; nothing happens at import beyond definitions.  A case is the input of one ``fdipt_ipa_attention_fwd`` call — ``node``, ``z``,
``rigids`` (quaternion, translation in A), ``res_mask`` and the block — plus what the tests need to know about it: the regime tag, the
planted keys and the case whose restatement is its reference.  The weights are the synthetic full-width network (``SEED``), blocks 0 and 3.
tests/test_ipa_attention_cases_host.py shows with the oracle alone that every case is in the regime it is tagged with and measures
DEV32 / EMU16; tests/test_gpu_ipa_attention_edges.py then asks the kernels.

The axes (a covering design, not a cross product: ``design()`` lists the rows):
  length    LENGTHS: ragged query tiles (a key tile is 32 keys, dealt round-robin to 4 waves), waves without a real key, one / two / three
            128-key stream chunks, the o_pair pass edge 320 | 324, and the smallest lengths of the <4,1>, <6,2>, <8,1> classes at B = 1
  batch     1, 2, 3 with a different mask per sample
  mask      ones | tail3 | lead32 | lead128 (the whole first stream chunk) | third (every third residue) | single (one real residue) |
            none (a sample masked entirely, beside two others)
  geometry  origin | walk (centred 3.8 A chain walk) | twochain (centroids 150 A apart) | shift (the walk moved by SHIFT: the module is
            invariant, so the reference is the restatement of the walk)
  sharpness diffuse | planted (query i, head i % 8: ALPHA w_h / |w_h| added to z[i, j*], the sum rounded to fp16; j* by PLANT_RULES) | tie (two planted keys of equal
            ALPHA in tiles of different waves and, at N > 128, different chunks) | masked (j* is a masked key: it must receive nothing)
"""
import functools

import numpy as np

F32 = np.float32
SEED = 7
BLOCKS = (0, 3)
H, C_S, C_Z = 8, 256, 128
LENGTHS = (1, 5, 31, 32, 33, 64, 65, 97, 128, 129, 160, 257, 320, 324)
LONG_LENGTHS = (388, 516, 772)
MASKS = ("ones", "tail3", "lead32", "lead128", "third", "single")
GEOMETRIES = ("origin", "walk", "twochain", "shift")
SHARPNESS = ("diffuse", "planted", "tie", "masked")
PLANT_RULES = ("key0", "last", "last_tile", "wave", "far128")
SHIFT = (60.0, -40.0, 30.0)  # A; inside the documented coordinate range of the fp16 point logits
# a plant adds sqrt(1/3) ALPHA |w_h| = 0.58 ALPHA to the logit (|w_h| = 1 within 10 % in the synthetic network); it has to beat the point term
# of the farthest pair, which the host test measures: up to 72 on the walks (N = 772) and 208 between the two chains
ALPHA = {"origin": 40.0, "walk": 160.0, "shift": 160.0, "twochain": 480.0}
TILE, WAVES, CHUNK = 32, 4, 128

# Measured by tests/test_ipa_attention_cases_host.py (which prints both tables and holds them to +-10 %): the worst per-row deviation
# max_c |a - b| / max_c |b| over the real rows of a regime's cases,
#   DEV32  float32 oracle against the float64 restatement,
#   EMU16  restatement with the fp16 mode's single-fp16 operands rounded (oracle.score_network.IPA_ROUND16) against the unrounded one.
DEV32 = {
    "diffuse/origin": 7.06e-07, "diffuse/shift": 3.59e-06, "diffuse/twochain": 1.28e-06, "diffuse/walk": 1.3e-06,
    "masked/origin": 6.17e-07, "masked/shift": 2.79e-06, "masked/twochain": 2.65e-06, "masked/walk": 1.05e-06,
    "planted/origin": 1.79e-06, "planted/shift": 1.46e-06, "planted/twochain": 1.66e-06, "planted/walk": 2.33e-06,
    "tie/origin": 4.25e-06, "tie/shift": 3.83e-06, "tie/twochain": 4e-06, "tie/walk": 3.15e-06,
}
EMU16 = {
    "diffuse/origin": 0.00023, "diffuse/shift": 0.000208, "diffuse/twochain": 0.000275, "diffuse/walk": 0.000237,
    "masked/origin": 0.000198, "masked/shift": 0.000273, "masked/twochain": 0.000282, "masked/walk": 0.000225,
    "planted/origin": 0.000301, "planted/shift": 0.000735, "planted/twochain": 0.0014, "planted/walk": 0.00109,
    "tie/origin": 0.000425, "tie/shift": 0.000799, "tie/twochain": 0.00144, "tie/walk": 0.00071,
}
CAP32, CAP16 = 3e-4, 4e-3  # the per-module tolerances of tests/test_gpu_sizes.py::test_per_module_entries_vs_oracle
FACTOR32, FACTOR16 = 8, 4


def bound(regime, half):
    """Per-row bound of a selection: the module tolerance, or the measured CPU deviation of the regime times the margin for another
    summation order and another draw of the rounding, whichever is smaller."""
    return min(CAP16, FACTOR16 * EMU16[regime]) if half else min(CAP32, FACTOR32 * DEV32[regime])


def row_error(a, b):
    """[..., rows]: max_c |a - b| / max_c |b| over the columns of a row (rows of zeros in ``b`` give inf unless ``a`` is zero too)."""
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    num, den = np.abs(a - b).max(-1), np.abs(b).max(-1)
    with np.errstate(divide="ignore", invalid="ignore"):
        return np.where(num == 0, 0.0, num / den)


def make_mask(kind, n):
    m = np.ones(n, dtype=F32)
    if kind == "tail3":
        m[n - 3:] = 0
    elif kind == "lead32":
        m[:32] = 0
    elif kind == "lead128":
        m[:128] = 0
    elif kind == "third":
        m[2::3] = 0
    elif kind == "single":
        m[:] = 0
        m[(2 * n) // 3] = 1
    elif kind == "none":
        m[:] = 0
    else:
        assert kind == "ones", kind
    return m


def mask_fits(kind, n):
    return {"ones": True, "tail3": n > 3, "lead32": n > 32, "lead128": n > 128, "third": n >= 3, "single": n >= 2, "none": True}[kind]


def _walk(rng, n):
    step = rng.standard_normal((n, 3))
    x = np.cumsum(3.8 * step / np.linalg.norm(step, axis=-1, keepdims=True), axis=0)
    return np.round((x - x.mean(0)) * 1024) / 1024  # (a 2^-10 A grid: adding SHIFT is exact in float32)


def make_trans(kind, rng, n):
    if kind == "origin":
        return np.zeros((n, 3))
    x = _walk(rng, n)
    if kind == "shift":
        return x + np.asarray(SHIFT)
    if kind == "twochain":
        h = n // 2
        a, b = x[:h] - (x[:h].mean(0) if h else 0), x[h:] - x[h:].mean(0)
        x = np.round(np.concatenate([a - [75.0, 0, 0], b + [75.0, 0, 0]]) * 1024) / 1024
    return x


def plant_keys(rule, i, mask):
    """Keys of query ``i`` under ``rule``; ``mask`` [N] of the sample.  None where the sample has no key the rule names."""
    n = len(mask)
    real = np.flatnonzero(mask > 0)
    tile, wave, chunk = (lambda j: j // TILE), (lambda j: (j // TILE) % WAVES), (lambda j: j // CHUNK)
    if len(real) == 0:
        return None
    if rule == "key0":
        return [int(real[0])]
    if rule == "last":
        return [int(real[-1])]
    if rule == "last_tile":  # a real key of the last (partial) tile, not the last real key where the tile holds another
        c = real[tile(real) == tile(n - 1)]
        return [int(c[(3 * i) % max(len(c) - 1, 1)])] if len(c) else None
    if rule == "wave":  # a tile of wave i % 4
        c = real[wave(real) == i % WAVES]
        return [int(c[(7 * i) % len(c)])] if len(c) else None
    if rule == "far128":  # another 128-key chunk than the query's, 128 keys away where the length allows
        c = real[chunk(real) != chunk(i)]
        if not len(c):
            return None
        want = i + CHUNK if i + CHUNK < n else i - CHUNK
        far = c[np.abs(c - i) >= CHUNK]
        c = far if len(far) else c
        return [int(c[np.argmin(np.abs(c - want))])]
    if rule == "tie":  # two keys: tiles of different waves and, where the sample has two chunks with real keys, different chunks
        tiles = np.unique(tile(real))
        two_chunks = len(np.unique(chunk(real))) > 1
        pairs = [(a, b) for a in tiles for b in tiles if a < b and a % WAVES != b % WAVES and (not two_chunks or a // WAVES != b // WAVES)]
        if not pairs:
            return None
        a, b = pairs[i % len(pairs)]
        ka, kb = real[tile(real) == a], real[tile(real) == b]
        return [int(ka[i % len(ka)]), int(kb[(5 * i) % len(kb)])]
    if rule == "masked":
        c = np.flatnonzero(mask == 0)
        return [int(c[(3 * i) % len(c)])] if len(c) else None
    raise KeyError(rule)


class Case:
    def __init__(self, name, n, masks, geom, sharp, rule, block, ref=None):
        self.name, self.N, self.B, self.masks, self.geom, self.sharp, self.rule, self.block = name, n, len(masks), masks, geom, sharp, rule, block
        self.regime = f"{sharp}/{geom}"
        self.ref = ref  # the case whose restatement is the reference (shift -> its walk twin, same draw); None: its own

    def __repr__(self):
        return self.name

    @functools.cached_property
    def arrays(self):
        return build(self)

    def drop(self):
        self.__dict__.pop("arrays", None)


@functools.lru_cache(maxsize=None)
def bias_rows():
    """{block: [H, c_z] float64} rows of linear_b of the synthetic network (the direction a plant is added along)."""
    from framedipt_amd import config
    from framedipt_amd import weights as W
    shapes = W.param_shapes(config.base_config().model)
    return {b: np.asarray(W.synth_tensor(f"score_model.trunk.ipa_{b}.linear_b.weight", shapes[f"score_model.trunk.ipa_{b}.linear_b.weight"],
                                          SEED, list(shapes).index(f"score_model.trunk.ipa_{b}.linear_b.weight")), dtype=np.float64)
            for b in BLOCKS}


def build(case):
    """dict(node [B,N,256], z [B,N,N,128], rigids [B,N,7], res_mask [B,N]: float32; plants: [(sample, query, head, [keys])])."""
    seed = [case.N, case.block, GEOMETRIES.index("walk" if case.geom == "shift" else case.geom)] + [(MASKS + ("none",)).index(m) for m in case.masks]
    rng = np.random.default_rng(seed)  # (a shift case draws what its walk draws)
    B, N = case.B, case.N
    node = rng.standard_normal((B, N, C_S)).astype(F32)
    z = rng.standard_normal((B, N, N, C_Z), dtype=F32)
    q = rng.standard_normal((B, N, 4))
    q /= np.linalg.norm(q, axis=-1, keepdims=True)
    trans = np.stack([make_trans(case.geom, rng, N) for _ in range(B)])
    mask = np.stack([make_mask(m, N) for m in case.masks])
    plants = []
    if case.sharp != "diffuse":
        w = bias_rows()[case.block]
        unit = (w / np.linalg.norm(w, axis=-1, keepdims=True)).astype(F32)
        rule = {"planted": case.rule, "tie": "tie", "masked": "masked"}[case.sharp]
        for s in range(B):
            for i in range(N):
                keys = plant_keys(rule, i, mask[s])
                if keys is None:
                    continue
                for j in keys:  # (the planted entry is an fp16 value: what the test plants is then what the fp16 mode reads, however large ALPHA)
                    z[s, i, j] = (z[s, i, j] + F32(ALPHA[case.geom]) * unit[i % H]).astype(np.float16).astype(F32)
                plants.append((s, i, i % H, keys))
    rig = np.concatenate([q, trans], axis=-1).astype(F32)
    return {"node": node, "z": z, "rigids": rig, "res_mask": mask, "plants": plants}


def _rot(seq, k):
    return seq[k % len(seq)]


@functools.lru_cache(maxsize=None)
def design():
    """The cases, in a fixed order.  Four rows per length: the geometries in turn, sharpness and masks rotated against them so that over the
    lengths every geometry meets every sharpness and every mask; batch sizes 1, 2, 3 in turn with another mask per sample; then the named
    pairings the rotation does not reach."""
    rows, names = [], set()

    def add(n, masks, geom, sharp, rule=None, block=None):
        masks = tuple(masks)
        assert all(mask_fits(m, n) for m in masks), (n, masks)
        block = BLOCKS[len(rows) % 2] if block is None else block
        name = f"n{n}-b{len(masks)}-{'+'.join(masks)}-{geom}-{sharp}" + (f"-{rule}" if rule else "") + f"-blk{block}"
        assert name not in names, name
        names.add(name)
        ref = None
        if geom == "shift":  # its walk twin: the same draw, not a case of its own unless the rotation made it one
            ref = Case(name.replace("-shift-", "-walk-"), n, masks, "walk", sharp, rule, block)
        rows.append(Case(name, n, masks, geom, sharp, rule, block, ref))

    for li, n in enumerate(LENGTHS):
        for c in range(4):
            geom = GEOMETRIES[c]
            sharp = _rot(SHARPNESS, c + li)
            fit = [m for m in MASKS if mask_fits(m, n)]
            with_zero = [m for m in fit if m not in ("ones",)]
            with_keys = [m for m in fit if m != "single"]
            if sharp == "masked" and not with_zero:
                sharp = "diffuse"
            if sharp == "tie" and n <= 2 * TILE:
                sharp = "planted" if n > 1 else "diffuse"
            pool = with_zero if sharp == "masked" else with_keys if sharp in ("planted", "tie") else fit
            if sharp == "tie":  # two real tiles of different waves must remain
                pool = [m for m in pool if plant_keys("tie", 0, make_mask(m, n)) is not None]
            nb = 1 if n >= 257 else 1 + (li + c) % 3
            masks = [_rot(pool, li + 2 * c + s) for s in range(nb)]
            rule = None
            if sharp == "planted":
                ok = [r for r in PLANT_RULES if all(plant_keys(r, i, make_mask(m, n)) is not None for m in masks for i in (0, n // 2, n - 1))
                      and (r != "wave" or n > 3 * TILE) and (r != "far128" or n > CHUNK) and (r != "last_tile" or n % TILE)]
                rule = _rot(ok, li + c)
            add(n, masks, geom, sharp, rule)
    # ---- named pairings
    add(65, ("ones", "tail3", "lead32"), "walk", "diffuse", block=0)          # nine query-tile groups over eight XCDs (fp32 kernel)
    add(97, ("third", "none", "ones"), "walk", "planted", "wave", block=3)    # a sample masked entirely beside two others
    add(33, ("ones", "none", "tail3"), "origin", "diffuse", block=0)
    add(257, ("lead128", "ones"), "walk", "planted", "far128", block=3)       # the whole first stream chunk masked; plants a chunk away
    add(160, ("lead128", "tail3"), "twochain", "diffuse", block=0)            # one real tile: three waves and a chunk without a real key
    add(257, ("lead128", "third"), "shift", "tie", block=3)
    add(129, ("ones", "third"), "origin", "planted", "last", block=0)         # the last real key alone in its tile and chunk
    add(128, ("single", "ones", "tail3"), "walk", "masked", block=3)
    add(324, ("third", "lead128"), "walk", "planted", "key0", block=0)
    add(320, ("ones",), "twochain", "planted", "far128", block=3)
    for n, sharp, rule, m, g in zip(LONG_LENGTHS, ("planted", "tie", "planted"), ("far128", None, "wave"), ("tail3", "lead128", "third"),
                                    ("walk", "origin", "walk")):
        add(n, (m,), g, sharp, rule)
    return tuple(rows)


@functools.lru_cache(maxsize=None)
def oracle_net():
    """The NumPy oracle on the synthetic full-width network (no residue tables: only its IPA is called)."""
    from framedipt_amd import config
    from framedipt_amd import weights as W
    from oracle import diffuser as od
    from oracle.score_network import ScoreNetwork
    conf = config.base_config()
    return ScoreNetwork(conf.model, od.SE3Diffuser(conf.diffuser), W.synth_state_dict(W.param_shapes(conf.model), SEED), tables=None)


def oracle_inputs(arrays, dtype):
    """(node, z, quat, trans in the network's units, mask) as ScoreNetwork.ipa takes them; the entry scales the translations by 0.1 in
    float32, the float64 restatement takes the float32 translations times 0.1 in float64."""
    rig = arrays["rigids"]
    trans = (rig[..., 4:] * F32(0.1)).astype(F32) if dtype == F32 else rig[..., 4:].astype(np.float64) * 0.1
    return arrays["node"], arrays["z"], rig[..., :4], trans, arrays["res_mask"]


def restate(case, round16=(), aux=False, own=False):
    """The float64 restatement on the case's reference inputs (a shift case: its walk; ``own``: the shifted inputs themselves), rows of masked
    residues zeroed as the entry does."""
    a = (case if own else case.ref or case).arrays
    node, z, quat, trans, mask = oracle_inputs(a, np.float64)
    r = oracle_net().ipa(case.block, node, z, quat, trans, mask, dtype=np.float64, round16=round16, aux=aux)
    out = (r[0] if aux else r) * mask[..., None]
    return (out, r[1]) if aux else out


def oracle32(case):
    """The float32 oracle on the case's own inputs, rows of masked residues zeroed."""
    node, z, quat, trans, mask = oracle_inputs(case.arrays, F32)
    return oracle_net().ipa(case.block, node, z, quat, trans, mask) * mask[..., None]


def by_name(name):
    return next(c for c in design() if c.name == name)
