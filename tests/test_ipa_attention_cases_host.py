"""tests/ipa_attention_cases.py on the CPU, with the oracle alone: the design covers its axes, every case is in the regime it is tagged
with (no row dropped), the logits leave the reference's -1e5 mask term unambiguous, the restatement is invariant under the rigid shift, and
the DEV32 / EMU16 tables the GPU bounds come from are what this file measures.  Also the argument errors of ``fdipt_ipa_attention_fwd`` that
are decided before the device is touched."""
import ctypes as C
import os

import numpy as np
import pytest

import ipa_attention_cases as ic
from oracle.score_network import IPA_ROUND16

TILE, WAVES, CHUNK = ic.TILE, ic.WAVES, ic.CHUNK


def test_design_covers_the_axes():
    d = ic.design()
    assert 56 <= len(d) <= 72 and len({c.name for c in d}) == len(d)
    assert {c.N for c in d} == set(ic.LENGTHS + ic.LONG_LENGTHS) and all(c.B == 1 for c in d if c.N in ic.LONG_LENGTHS)
    assert {c.B for c in d} == {1, 2, 3} and {c.block for c in d} == set(ic.BLOCKS)
    assert {m for c in d for m in c.masks} == set(ic.MASKS) | {"none"}
    assert {c.geom for c in d} == set(ic.GEOMETRIES) and {c.sharp for c in d} == set(ic.SHARPNESS)
    assert {c.rule for c in d if c.sharp == "planted"} == set(ic.PLANT_RULES)
    pairs = lambda f, g: {(f(c), g(c)) for c in d}  # noqa: E731
    assert pairs(lambda c: c.geom, lambda c: c.sharp) == {(g, s) for g in ic.GEOMETRIES for s in ic.SHARPNESS}
    gm = {(c.geom, m) for c in d for m in c.masks}
    assert all((g, m) in gm for g in ic.GEOMETRIES for m in ic.MASKS), sorted({(g, m) for g in ic.GEOMETRIES for m in ic.MASKS} - gm)
    assert any(c.N == 65 and c.B == 3 for c in d)                                        # nine query-tile groups over eight XCDs
    assert any(c.B == 3 and "none" in c.masks for c in d)                                # a sample masked entirely beside two others
    assert any(c.N > 128 and "lead128" in c.masks and c.sharp == "planted" and c.rule == "far128" for c in d)
    assert any(c.sharp == "tie" and c.N > 128 for c in d) and any(c.sharp == "tie" and c.N <= 128 for c in d)
    assert all(len(set(c.masks)) == c.B or c.N == 1 for c in d)                          # another mask per sample
    assert all(set(np.unique(ic.make_mask(m, c.N))) <= {0.0, 1.0} for c in d for m in c.masks)
    assert {c.regime for c in d} == set(ic.DEV32) == set(ic.EMU16)


def _check_plants(case, a):
    """The keys a rule names lie where the rule says (index arithmetic only)."""
    mask = a["res_mask"]
    tile, wave, chunk = (lambda j: j // TILE), (lambda j: (j // TILE) % WAVES), (lambda j: j // CHUNK)
    n = case.N
    assert (case.sharp == "diffuse") == (len(a["plants"]) == 0) or all(m in ("none",) for m in case.masks)
    for s, i, h, keys in a["plants"]:
        real = np.flatnonzero(mask[s] > 0)
        assert h == i % ic.H
        if case.sharp == "masked":
            assert all(mask[s, j] == 0 for j in keys)
            continue
        assert all(mask[s, j] == 1 for j in keys)
        if case.sharp == "tie":
            j1, j2 = keys
            assert wave(j1) != wave(j2) and (len(np.unique(chunk(real))) == 1 or chunk(j1) != chunk(j2))
        elif case.rule == "key0":
            assert keys == [real[0]]
        elif case.rule == "last":
            assert keys == [real[-1]]
        elif case.rule == "last_tile":
            assert n % TILE and tile(keys[0]) == tile(n - 1)
        elif case.rule == "wave":
            assert wave(keys[0]) == i % WAVES
        elif case.rule == "far128":
            assert chunk(keys[0]) != chunk(i)
    for s, kind in enumerate(case.masks):  # the all-masked tile, chunk or sample exists
        if kind == "lead32":
            assert not mask[s, :TILE].any() and mask[s, TILE:].all()
        if kind == "lead128":
            assert not mask[s, :CHUNK].any() and mask[s, CHUNK:].all()
        if kind == "single":
            assert mask[s].sum() == 1
        if kind == "none":
            assert not mask[s].any()


@pytest.fixture(scope="module")
def measured():
    """One pass over the design: per case the float64 restatement (with logits and weights), the float32 oracle and the rounded restatement."""
    rec = {}
    for case in ic.design():
        a = case.arrays
        _check_plants(case, a)
        mask = a["res_mask"]
        real = mask > 0
        ref, aux = ic.restate(case, aux=True)
        assert np.isfinite(ref).all() and (ref[~real] == 0).all()
        e32 = ic.row_error(ic.oracle32(case), ref)[real]
        e16 = ic.row_error(ic.restate(case, IPA_ROUND16), ref)[real]
        pair = np.broadcast_to(((mask[:, :, None] * mask[:, None, :]) > 0)[:, None], aux["logits"].shape)
        w = aux["weights"]
        plant = np.array([[sum(w[s, h, i, j] for j in keys), min(w[s, h, i, j] for j in keys)] for s, i, h, keys in a["plants"] if mask[s, i] > 0]).reshape(-1, 2)
        shift = float(ic.row_error(ic.restate(case, own=True), ref).max()) if case.geom == "shift" else 0.0
        # the weights a real query gives to masked keys: exactly zero in the restatement (exp(-1e5) underflows)
        leak = float((w * (real[:, None, :, None] & ~real[:, None, None, :])).max())
        rec[case.name] = dict(dev32=float(e32.max()) if e32.size else 0.0, emu16=float(e16.max()) if e16.size else 0.0,
                              logit=float(np.abs(aux["logits"][pair]).max()) if pair.any() else 0.0, plant=plant, shift=shift, leak=leak)
        case.drop()
        if case.ref is not None:
            case.ref.drop()
    return rec


def test_every_case_has_the_regime_it_is_tagged_with(measured):
    balanced = {}
    for case in ic.design():
        r = measured[case.name]
        assert r["leak"] == 0.0, case
        if case.sharp in ("planted", "tie"):
            assert len(r["plant"]) and r["plant"][:, 0].min() > 0.99, (case, r["plant"][:, 0].min())
        if case.sharp == "planted" and case.rule == "key0":
            balanced.setdefault("key0 is key 0", []).append(case.masks[0] in ("ones", "tail3", "third"))
        if case.sharp == "tie":  # equal plants, unequal point terms: rows where both keys keep more than a tenth
            balanced[case.name] = int((r["plant"][:, 1] > 0.1).sum())
        if case.sharp == "masked":
            assert len(r["plant"]) and r["plant"].max() == 0.0, case
    assert any(balanced.pop("key0 is key 0"))
    print("tie cases, rows in which both planted keys hold more than 0.1:", balanced)
    assert all(v >= 4 for v in balanced.values()), balanced


def test_unmasked_logits_stay_below_1e3(measured):
    """The reference's mask term is -1e5: with every logit of a real pair below 1e3 in magnitude it decides alone.  The two-chain geometry
    has the largest point terms (and the largest plants)."""
    worst = {g: max(measured[c.name]["logit"] for c in ic.design() if c.geom == g) for g in ic.GEOMETRIES}
    print("largest |logit| of a real pair per geometry:", {g: round(v, 1) for g, v in worst.items()})
    assert all(v < 1e3 for v in worst.values()) and worst["twochain"] == max(worst.values())


def test_restatement_is_invariant_under_the_rigid_shift(measured):
    worst = max(measured[c.name]["shift"] for c in ic.design() if c.geom == "shift")
    print(f"restatement of the shifted inputs against that of the walk: worst row {worst:.2e}")
    assert sum(c.geom == "shift" for c in ic.design()) >= 10 and worst < 1e-12


def test_tables_are_what_this_file_measures(measured):
    dev, emu = {}, {}
    for case in ic.design():
        r = measured[case.name]
        dev[case.regime], emu[case.regime] = max(dev.get(case.regime, 0.0), r["dev32"]), max(emu.get(case.regime, 0.0), r["emu16"])
    fmt = lambda t: "{" + ", ".join(f'"{k}": {v:.3g}' for k, v in sorted(t.items())) + "}"  # noqa: E731
    print("DEV32 =", fmt(dev))
    print("EMU16 =", fmt(emu))
    for name, got, want in (("DEV32", dev, ic.DEV32), ("EMU16", emu, ic.EMU16)):
        assert set(got) == set(want), name
        for k in got:
            assert 0.9 * want[k] <= got[k] <= 1.1 * want[k], (name, k, got[k], want[k])


def test_float64_switch_leaves_the_float32_path_alone():
    """The defaults of ScoreNetwork.ipa stay the float32 arithmetic (tests/test_oracle_forward.py holds it to the reference goldens), the
    rounding hooks and the auxiliary outputs belong to the float64 path, and unknown hooks are refused."""
    case = ic.by_name("n33-b2-single+ones-origin-diffuse-blk0")
    node, z, quat, trans, mask = ic.oracle_inputs(case.arrays, np.float32)
    net = ic.oracle_net()
    out = net.ipa(case.block, node, z, quat, trans, mask)
    assert out.dtype == np.float32
    with pytest.raises(AssertionError):
        net.ipa(case.block, node, z, quat, trans, mask, round16=("z",))
    with pytest.raises(AssertionError):
        net.ipa(case.block, node, z, quat, trans, mask, dtype=np.float64, round16=("v",))
    o64, aux = net.ipa(case.block, node, z, quat, trans, mask, dtype=np.float64, aux=True)
    assert o64.dtype == np.float64 and set(aux) == {"logits", "weights", "feats"}
    assert aux["feats"].shape == (case.B, case.N, net.sd[f"score_model.trunk.ipa_{case.block}.linear_out.weight"].shape[1])
    assert aux["logits"].shape == aux["weights"].shape == (case.B, ic.H, case.N, case.N)
    np.testing.assert_allclose(aux["weights"].sum(-1), 1.0, atol=1e-14)


def check_argument_errors(lib):
    """block out of range, null pointers, a workspace too small: decided on the host values, before the device is touched (the pointers
    are never read)."""
    from framedipt_amd import _lib, config
    from framedipt_amd.model.score_network import dims_from_conf
    conf = config.base_config()
    dims = dims_from_conf(conf.model, conf.diffuser, False, _lib.PREC_F16, 0)
    B, N = 2, 33
    nb = lib.fdipt_forward_workspace_bytes(C.byref(dims), B, N)
    assert nb > 0
    buf = C.create_string_buffer(64)
    p = C.c_void_p(C.addressof(buf))
    good = dict(params=p, derived=p, block=0, node=p, z=p, rigids=p, res_mask=p, out=p, workspace=p, workspace_bytes=nb)

    def call(**kw):
        a = dict(good, **kw)
        return lib.fdipt_ipa_attention_fwd(C.byref(dims), a["params"], a["derived"], a["block"], B, N, a["node"], a["z"], a["rigids"], a["res_mask"],
                                           a["out"], a["workspace"], a["workspace_bytes"], None)

    assert call(block=-1) == call(block=conf.model.ipa.num_blocks) == _lib.EINVAL
    for k in ("params", "derived", "rigids", "res_mask", "workspace"):
        assert call(**{k: None}) == _lib.EINVAL, k
    assert call(workspace_bytes=nb - 1) == call(workspace_bytes=0) == _lib.ESIZE
    assert lib.fdipt_ipa_attention_fwd(None, p, p, 0, B, N, p, p, p, p, p, p, nb, None) == _lib.EINVAL


def test_argument_errors_decided_on_the_host():
    from framedipt_amd import _lib
    assert os.path.exists(_lib.LIB_PATH), "run __graft_entry__.build() first"
    check_argument_errors(_lib.load())
