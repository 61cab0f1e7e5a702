"""CPU tests of framedipt_amd/_call.py, the call path the sample-analysis entries share: pair planning, the shape errors every public
entry raises before torch.cuda or the library is touched, and the per-row helper's mismatch message."""
import numpy as np
import pytest

from framedipt_amd import _call


def test_plan_pairs_routes():
    pairs, square = _call.plan_pairs(4, 4, False, None, None)                      # all-against-all
    assert square and pairs.dtype == np.int32 and pairs.tolist() == [[0, 1], [0, 2], [0, 3], [1, 2], [1, 3], [2, 3]]
    pairs, square = _call.plan_pairs(1, 1, False, None, None)                      # one structure: no pair, still square
    assert square and pairs.shape == (0, 2) and pairs.dtype == np.int32
    pairs, square = _call.plan_pairs(3, 3, True, None, None)                       # prot_b with S_b = S: row i
    assert not square and pairs.tolist() == [[0, 0], [1, 1], [2, 2]]
    pairs, square = _call.plan_pairs(3, 1, True, None, None)                       # prot_b with S_b = 1: row 0
    assert not square and pairs.tolist() == [[0, 0], [1, 0], [2, 0]]
    pairs, square = _call.plan_pairs(1, 1, True, None, None)
    assert not square and pairs.tolist() == [[0, 0]]
    for has_b, s_b in ((True, 5), (False, 3)):                                     # explicit ref_index, with and without prot_b
        pairs, square = _call.plan_pairs(3, s_b, has_b, None, np.array([2, 0, 1]))
        assert not square and pairs.dtype == np.int32 and pairs.tolist() == [[0, 2], [1, 0], [2, 1]]
    pairs, square = _call.plan_pairs(3, 3, False, [[2, 1], [0, 0]], None)          # explicit pairs: as listed
    assert not square and pairs.dtype == np.int32 and pairs.tolist() == [[2, 1], [0, 0]]
    pairs, square = _call.plan_pairs(3, 2, True, np.array([0, 1, 2, 1]), np.array([9, 9, 9]))  # pairs win over ref_index; flat lists fold
    assert not square and pairs.tolist() == [[0, 1], [2, 1]]
    with pytest.raises(ValueError, match="holds 2 structures for 3 samples"):
        _call.plan_pairs(3, 2, True, None, None)


def test_square_matrix_mirrors_and_keeps_the_unit_diagonal():
    pairs = _call.all_pairs(3)
    m = _call.square_matrix(3, pairs, np.array([0.25, 0.5, 0.75]))
    assert m.dtype == np.float64 and m.tolist() == [[1.0, 0.25, 0.5], [0.25, 1.0, 0.75], [0.5, 0.75, 1.0]]
    assert _call.square_matrix(1, _call.all_pairs(1), np.zeros(0)).tolist() == [[1.0]]


def _entries():
    from framedipt_amd import evaluation, inverse_folding, sasa, secondary_structure, selection, tm_align, tm_score, violations
    model = inverse_folding.ProteinMPNN()
    mask = lambda x: np.ones(x.shape[:2], np.float32)  # noqa: E731
    letters = lambda x: np.zeros(x.shape[:2], np.int64)  # noqa: E731
    return {"select_samples": lambda x: selection.select_samples(x, mask(x)),
            "evaluate_samples": lambda x: evaluation.evaluate_samples(x, x, mask(x)),
            "structural_violations": violations.structural_violations,
            "secondary_structure": secondary_structure.secondary_structure,
            "solvent_accessibility": sasa.solvent_accessibility,
            "tm_scores": tm_score.tm_scores,
            "tm_scores_b": lambda x: tm_score.tm_scores(np.zeros((2, 4, 37, 3), np.float32), x),
            "tm_align": tm_align.tm_align,
            "tm_align_b": lambda x: tm_align.tm_align(np.zeros((2, 4, 37, 3), np.float32), x),
            "mpnn_score": lambda x: model.score(x, letters(x)),
            "mpnn_design": model.design,
            "mpnn_unconditional_probs": model.unconditional_probs,
            "mpnn_conditional_probs": lambda x: model.conditional_probs(x, letters(x))}


ENTRIES = ("select_samples", "evaluate_samples", "structural_violations", "secondary_structure", "solvent_accessibility", "tm_scores",
           "tm_scores_b", "tm_align", "tm_align_b", "mpnn_score", "mpnn_design", "mpnn_unconditional_probs", "mpnn_conditional_probs")


@pytest.mark.parametrize("entry", ENTRIES)
def test_entries_raise_their_shape_errors_before_the_device(entry, monkeypatch):
    """36 atoms and an empty batch are refused from ``.shape`` alone: neither torch.cuda nor the library is asked."""
    import torch

    from framedipt_amd import _lib

    def touched(*args, **kwargs):
        raise AssertionError("the shape check came after the device or the library")

    for name in ("current_device", "is_available", "device_count", "current_stream"):
        monkeypatch.setattr(torch.cuda, name, touched)
    monkeypatch.setattr(_lib, "load", touched)
    call = _entries()[entry]
    with pytest.raises(ValueError, match=r"37, 3\]"):
        call(np.zeros((2, 4, 36, 3), np.float32))
    for shape in ((0, 4, 37, 3), (2, 0, 37, 3)):
        with pytest.raises(ValueError, match="no residues"):
            call(np.zeros(shape, np.float32))


def test_structure_shape_reads_shape_only():
    class Shaped:
        shape = (3, 7, 5, 3)

    assert _call.structure_shape(Shaped()) == (3, 7, 5)
    with pytest.raises(ValueError, match=r"prot should be \[B, N, 37, 3\], got \(3, 7, 5, 3\)"):
        _call.structure_shape(Shaped(), atoms=(37,))
    with pytest.raises(ValueError, match=r"prot_b should be \[S, N, 37, 3\] or \[S, N, 5, 3\], got \(2, 4, 3\)"):
        _call.structure_shape(np.zeros((2, 4, 3)), "prot_b", lead="S")
    with pytest.raises(ValueError, match="no structures or no residues"):
        _call.structure_shape(np.zeros((0, 4, 5, 3)), "prot_a", items="structures")


def test_per_row_on_the_host():
    x = np.array([[0.0, 2.0, -1.0], [0.4, 0.0, 1.6]])
    mask = _call.per_row(x, (2, 3), "res_mask", "mask")
    assert mask.dtype == np.float32 and mask.flags.c_contiguous and mask.tolist() == [[0, 1, 1], [1, 0, 1]]
    index = _call.per_row(x, (2, 3), "chain_idx", "int")                            # floats are rounded, not truncated
    assert index.dtype == np.int32 and index.tolist() == [[0, 2, -1], [0, 0, 2]]
    assert _call.per_row(np.array([[7, 8]], np.int64), (1, 2), "residue_index", "int").dtype == np.int32
    assert _call.per_row(x, (2, 3), "aatype") .dtype == np.float64                  # raw: as given
    ones = _call.per_row(None, (2, 3), "res_mask", "mask", default=1)
    assert ones.dtype == np.float32 and ones.shape == (2, 3) and (ones == 1).all()
    zeros = _call.per_row(None, (2, 3), "chain_idx", "int", default=0)
    assert zeros.dtype == np.int32 and not zeros.any()
    assert _call.per_row(None, (2, 3), "residue_index", "int") is None
    import torch
    assert _call.per_row(torch.tensor(x), (2, 3), "res_mask", "mask").tolist() == mask.tolist()  # a tensor comes to the host


@pytest.mark.parametrize("kind", ("mask", "int", "raw"))
def test_per_row_mismatch_names_the_input_and_both_shapes(kind):
    with pytest.raises(ValueError, match=r"align_mask \(2, 4\) does not match prot: expected \(2, 3\)"):
        _call.per_row(np.zeros((2, 4)), (2, 3), "align_mask", kind, default=1)
    with pytest.raises(ValueError, match=r"atom_mask \(2, 3\) does not match prot: expected \(2, 3, 5\)"):
        _call.per_row(np.zeros((2, 3)), (2, 3, 5), "atom_mask", kind)


def test_check_shapes_keeps_both_message_tails_and_needs_no_torch(monkeypatch):
    import sys
    monkeypatch.setitem(sys.modules, "torch", None)  # (an import of torch would raise)
    wrong = np.ones((2, 9))
    checks = (("res_mask", None, (1, 7)), ("res_mask_b", wrong, (1, 9)), ("atom_mask_b", np.ones((3, 3)), (1, 9, 5)))  # (the first mismatch is named)
    with pytest.raises(ValueError, match=r"res_mask_b \(2, 9\) does not match prot: expected \(1, 9\)"):
        _call.check_shapes(checks)
    with pytest.raises(ValueError, match=r"res_mask_b \(2, 9\) does not match its structure: expected \(1, 9\)"):
        _call.check_shapes(checks, mapped=True)
    with pytest.raises(ValueError, match=r"res_mask_b \(2, 9\) does not match"):
        _call.check_shapes((("res_mask_b", wrong.tolist(), [1, 9]),))          # a nested list has a shape too; the expected shape may be a list
    _call.check_shapes((("res_mask", None, (1, 7)), ("res_mask_b", wrong, (2, 9))))
    _call.check_shapes(())


def test_the_folded_entries_keep_each_message_tail_where_it_was(monkeypatch):
    import sys
    monkeypatch.setitem(sys.modules, "torch", None)  # (an import of torch would raise)
    from framedipt_amd import interface, lddt
    wrong = np.ones((2, 9))
    a, b, side = np.ones((1, 7, 3), np.float32), np.ones((1, 9, 3), np.float32), np.array([1] * 4 + [2] * 5)
    for call in (lambda **kw: interface.interface_accuracy(a, b, side, atoms="ca", **kw), lambda **kw: lddt.local_accuracy(a, b, **kw)):
        with pytest.raises(ValueError, match=r"res_mask_b \(2, 9\) does not match its structure: expected \(1, 9\)"):
            call(alignment=np.full(9, -1), res_mask_b=wrong)
    with pytest.raises(ValueError, match=r"res_mask_b \(2, 9\) does not match prot: expected \(1, 9\)"):
        interface.interface_accuracy(b, b, side, atoms="ca", res_mask_b=wrong)


def test_add_coverage_and_its_result_without_a_call():
    assert _call.add_coverage({"n_covered": np.array([2, 0]), "n_reference": np.array([4, 0])}, 2)["coverage"].tolist() == [0.5, 0.0]
    empty = _call.add_coverage({}, 0)
    assert {k: (v.dtype, v.shape) for k, v in empty.items()} == {k: (np.dtype(t), (0,)) for k, t in (("n_covered", "int64"), ("n_reference", "int64"), ("coverage", "float64"))}


def test_outputs_without_a_call():
    spec = {"tm": ("float64", (0,)), "rotation": ("float64", (0, 3, 3)), "status": ("int32", (0,))}
    out = _call.empty_outputs(spec, widen=("status",))
    assert {k: (v.dtype, v.shape) for k, v in out.items()} == {"tm": (np.float64, (0,)), "rotation": (np.float64, (0, 3, 3)), "status": (np.int64, (0,))}
