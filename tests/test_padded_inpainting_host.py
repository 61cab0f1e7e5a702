"""Host side (no GPU) of the padded inpainting path: sharding.pad_item / stack_items_padded on the conditional sampler's complete key
set, the fixtures of tests/golden/make_goldens_padded.py, and the edge embedder's row-table predicate at the shapes
tests/test_gpu_padded_inpainting.py runs."""
import ctypes as C
import zlib

import numpy as np
import pytest
import torch

from conftest import load_golden
from padded_inpainting_cases import FIXTURES, PAIRS, PER_RESIDUE, SAMPLER_KEYS, hand_item


@pytest.mark.parametrize("n,n_pad", [(45, 48), (7, 8)])
def test_pad_item_on_the_conditional_samplers_key_set(n, n_pad):
    """Every key ConditionalSampler hands over, plus a non-tensor entry, through pad_item.  N = 7 collides with the width of a frame
    ([1, 7, 7]) and with the torsion axis ([1, 7, 7, 2]): still axis 1 only."""
    from framedipt_amd import sharding
    feats, tape = hand_item(n, seed=n)
    assert set(SAMPLER_KEYS) < set(feats) and not torch.is_tensor(feats["pdb_name"])
    before = {k: v.clone() if torch.is_tensor(v) else v for k, v in feats.items()}
    out, tape_p = sharding.pad_item(feats, tape, n_pad)
    assert set(out) == set(feats)
    for k, v in before.items():
        if k in PER_RESIDUE:
            assert tuple(out[k].shape) == (1, n_pad) + tuple(v.shape[2:]), k   # grows on axis 1 only
            assert out[k].dtype == v.dtype, k
            assert torch.equal(out[k][:, :n], v), k                            # real rows: bit-identical
        else:
            assert out[k] is feats[k], k                                       # passed through by identity
        if torch.is_tensor(v):
            assert torch.equal(feats[k], v), k                                 # the input dict is not written
    pad = slice(n, n_pad)
    res_mask, fixed = out["res_mask"], out["fixed_mask"]
    assert float(res_mask[:, pad].abs().sum()) == 0 and float(fixed[:, pad].abs().sum()) == 0
    assert float((((1 - fixed) * res_mask)[:, pad]).abs().sum()) == 0 and float(((fixed * res_mask)[:, pad]).abs().sum()) == 0
    ident = torch.tensor([1.0, 0, 0, 0, 0, 0, 0])
    assert torch.equal(out["rigids_t"][0, pad], ident.expand(n_pad - n, 7))
    assert torch.equal(out["seq_idx"][0, pad], feats["seq_idx"][0, -1:].expand(n_pad - n))
    assert int(out["seq_idx"].max() - out["seq_idx"].min()) == int(feats["seq_idx"].max() - feats["seq_idx"].min())
    assert ((out["aatype"][0, pad] >= 0) & (out["aatype"][0, pad] <= 20)).all()
    assert ((out["chain_idx"][0, pad] >= 0) & (out["chain_idx"][0, pad] <= int(feats["chain_idx"].max()))).all()
    for k in PER_RESIDUE:
        assert torch.isfinite(out[k].double()).all(), k
    for z, zp in zip(tape, tape_p):
        assert zp.shape == z.shape[:2] + (n_pad, 3) and zp.dtype == z.dtype
        np.testing.assert_array_equal(zp[:, :, :n], z)
        assert not zp[:, :, n:].any()
    # a noise key (device noise) or None in the tape's place passes through; so does a dict that needs no padding
    assert sharding.pad_item(feats, 1234, n_pad)[1] == 1234 and sharding.pad_item(feats, None, n_pad)[1] is None
    same, same_tape = sharding.pad_item(feats, tape, n)
    assert same is feats and same_tape is tape
    with pytest.raises(ValueError):
        sharding.pad_item(feats, tape, n - 1)


def test_stack_items_padded_on_two_inpainting_items():
    """Lengths 45 and 42: common length 48, every sample keeps its own rows, seq_idx and fixed_mask."""
    from framedipt_amd import sharding
    items = [("a", 0) + hand_item(45, seed=1), ("b", 0) + hand_item(42, seed=2, gap=20)]
    tensor_keys = [k for k in items[0][2] if torch.is_tensor(items[0][2][k])]
    feats, tape, lengths = sharding.stack_items_padded([(a, b, {k: f[k] for k in tensor_keys}, t) for a, b, f, t in items])
    assert lengths == [45, 42]
    for b, (_, _, f, t) in enumerate(items):
        n = lengths[b]
        for k in PER_RESIDUE:
            assert tuple(feats[k].shape) == (2, 48) + tuple(f[k].shape[2:]), k
            assert torch.equal(feats[k][b, :n], f[k][0]), (b, k)
        assert float(feats["res_mask"][b, n:].abs().sum()) == 0 and float(feats["fixed_mask"][b, n:].abs().sum()) == 0
        assert (feats["seq_idx"][b, n:] == f["seq_idx"][0, -1]).all()
        for j in range(2):
            assert tape[j].shape == (3, 2, 48, 3)
            np.testing.assert_array_equal(tape[j][:, b, :n], t[j][:, 0])
            assert not tape[j][:, b, n:].any()
    assert tuple(feats["t"].shape) == (2,)
    assert not torch.equal(feats["seq_idx"][0, :42], feats["seq_idx"][1, :42])
    assert not torch.equal(feats["fixed_mask"][0], feats["fixed_mask"][1])


def test_fixtures_are_what_the_gpu_tests_assume():
    """The four fixtures: the keys of the N = 40 fixture, two chains with the stated gap, one diffused window per chain, GLY among the
    residues (the zero pattern of CB bites), different seeds and chain splits within a pair."""
    ref_keys = set(load_golden("traj_full_inpaint_n40_T4_aatype.npz"))
    for name, (n, gap, n_alone, n_rel) in FIXTURES.items():
        G = load_golden(f"traj_{name}.npz")
        assert set(G) == ref_keys, name
        assert int(G["num_t"]) == 4 and float(G["min_t"]) == 0.01 and float(G["noise_scale"]) == 0.1 and int(G["input_aatype"]) == 1
        assert n % 4 != 0 and n_alone == -(-n // 4) * 4
        seq, chain, fixed = G["in_seq_idx"][0], G["in_chain_idx"][0], G["in_fixed_mask"][0]
        n1 = n // 2
        assert seq.shape == (n,) and (np.diff(seq) == np.where(np.arange(n - 1) == n1 - 1, gap + 1, 1)).all()
        assert 2 * int(seq.max() - seq.min()) + 1 == n_rel
        assert (chain[:n1] == 0).all() and (chain[n1:] == 1).all()
        assert 0 < (fixed[:n1] == 0).sum() < n1 and 0 < (fixed[n1:] == 0).sum() < n - n1 and (G["in_res_mask"] == 1).all()
        assert (G["in_aatype"] == 7).any()
        assert G["noise_tape"].shape == (6, 1, n, 3) and G["res_prot_traj"].shape == (4, 1, n, 37, 3)
        assert G["res_rigid_traj"].shape == (5, 1, n, 7) and G["res_psi_pred"].shape == (1, 1, n, 2)
    for a, b, n_pad in PAIRS.values():
        assert zlib.crc32(a.encode()) % 1000 != zlib.crc32(b.encode()) % 1000
        assert FIXTURES[a][0] // 2 != FIXTURES[b][0] // 2 and n_pad == FIXTURES[a][2] and FIXTURES[b][2] < n_pad


@pytest.mark.parametrize("prec", ["fp16", "fp16x"])
def test_row_table_predicate_at_the_shapes_of_the_gpu_tests(prec):
    """fdipt_embed_table_rows at the shapes of the N = 126 / 122 fixtures (chain gap 20: n_rel = 291 / 283) and of the N = 45 / 42 ones.
    A network WITHOUT aatype features (the de novo model: its pair features depend on the fixed-mask bits, rel and the distogram bin
    only) takes the table for the padded N = 126 / 122 shapes, alone and as a batch, and declines the N = 45 / 42 ones and every
    unpadded length.  The inpainting model embeds aatype (use_aatype = 1: 21 x 21 more classes per pair), so the predicate declines
    it at EVERY shape: the reference-pinned inpainting runs of test_gpu_padded_inpainting.py evaluate every pair, and the table path
    is run on the same mixed, padded features by the de novo network of
    test_row_table_on_a_mixed_padded_batch_equals_the_pair_kernel there."""
    from framedipt_amd import _lib, config
    from framedipt_amd.model.score_network import dims_from_conf
    code = {"fp16": _lib.PREC_F16, "fp16x": _lib.PREC_F16X}[prec]

    def rows_of(inpainting):
        conf = config.base_config(inpainting=inpainting)
        d = dims_from_conf(conf.model, conf.diffuser, inpainting, code)
        assert d.num_bins == 22 and d.use_aatype == int(inpainting)
        return lambda b, n, n_rel: int(_lib.load().fdipt_embed_table_rows(C.byref(d), b, n, n_rel))

    rows = rows_of(False)
    assert rows(2, 128, 291) == 291 * 23 and rows(1, 128, 291) == 291 * 23 and rows(1, 124, 283) == 283 * 23
    assert rows(1, 136, 291) == 291 * 23
    assert rows(2, 48, 489) == 0 and rows(1, 48, 489) == 0 and rows(1, 44, 483) == 0 and rows(1, 56, 489) == 0
    assert rows(1, 126, 291) == 0 and rows(1, 122, 283) == 0
    rows = rows_of(True)
    for shape in ((2, 128, 291), (1, 128, 291), (1, 124, 283), (1, 136, 291), (2, 48, 489), (1, 48, 489)):
        assert rows(*shape) == 0, shape
