"""CPU tests of run_sharded's rank-0 analysis driver: the batch helpers on hand-made gathered entries, the stage plan of ``main()`` as a
truth table, and the pure-host writers byte for byte against tests/golden/run_sharded_writers/ (written by the functions as they were
before the shared writers existed, from the inputs of ``writer_inputs`` below: ``write_all(<directory>)`` regenerates them)."""
import os

import numpy as np
import pytest

from framedipt_amd import run_sharded

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "run_sharded_writers")
NAN = float("nan")


# ---- the writers ------------------------------------------------------------------------------------------------------------------

def symmetric(n, seed):
    """[n,n] float64 in (0, 1), symmetric, unit diagonal: a score matrix."""
    m = np.random.default_rng(seed).uniform(0.2, 0.9, (n, n))
    m = (m + m.T) / 2
    np.fill_diagonal(m, 1.0)
    return m


def writer_inputs():
    """The fixed inputs of the six writers: 3 x 3 and 4 x 4 matrices, one NaN score, one skipped name, two lengths."""
    three, four = symmetric(3, 1), symmetric(4, 2)
    holed = four.copy()
    holed[0, 3] = holed[3, 0] = NAN  # (the search gave no score: the fixed one stands in)
    lower = np.float32(0.5) * four.astype(np.float32)
    lower[1, 2] = lower[2, 1] = np.float32(0.95)  # (one pair where the fixed correspondence wins)
    blind = three.astype(np.float32)
    blind[0, 1] = blind[1, 0] = NAN  # (a pair without either score: the length is written but not clustered)
    fixed = {"gdt_ts": np.array([0.5, NAN, 0.25], np.float32), "gdt_ha": np.array([0.375, NAN, 0.125], np.float32)}
    search = {"gdt_ts": np.array([0.75, 0.625, NAN], np.float32), "gdt_ha": np.array([0.5, 0.4375, NAN], np.float32)}
    counts = np.arange(15, dtype=np.int32).reshape(3, 5)
    return {
        "gdt": dict(structures={"1abc": {"samples": ["0", "1", "mean"], "n_scored": np.array([12, 12, 11]), "fixed": fixed, "search": search,
                                         "counts_fixed": counts, "counts": counts + 1, "status": np.array([0, 2, 4], np.int32)}}, skipped=["2xyz"]),
        "tm_table": dict(structures={"1abc": {"samples": ["0", "1", "2"], "tm_score": np.array([0.71, NAN, 0.33], np.float32), "n_aligned": np.array([10, 2, 10]),
                                              "matrix": three.astype(np.float32)},
                                     "3def": {"samples": ["0", "1", "2", "3"], "tm_score": np.full(4, NAN), "n_aligned": np.array([7, 7, 7, 7]), "matrix": holed}}),
        "diversity": dict(matrices={4: four.astype(np.float32), 3: three}, tm_score_th=0.6),
        "diversity_aligned": dict(aligned={4: holed, 3: blind}, fixed={4: lower, 3: np.full((3, 3), NAN)}, tm_score_th=0.5, skipped=[900], inits="all"),
        "tm_align_table": dict(structures={"1abc": {"samples": ["0", "1", "2"], "rows": np.int64(14), "matrix": three.astype(np.float32)},
                                           "3def": {"samples": ["0", "1", "2", "3"], "rows": 9, "matrix": holed}}, skipped={"2xyz": 700}, inits="all"),
        "seq_diversity": dict(owners=[("a_sample_0", 0), ("a_sample_0", 1), ("b_sample_0", 0), ("b_sample_0", 1)], matrix=four,
                              scoring={"matrix": "blosum62", "open_gap": -10.0, "extend_gap": -0.5, "mode": "local"}, matrix_file="pairwise_seq_identity_local.npy"),
    }


def write_all(out_dir):
    """Every pure-host writer into ``out_dir``."""
    inputs = writer_inputs()
    run_sharded.write_gdt(out_dir, **inputs["gdt"])
    run_sharded.write_tm_table(out_dir, **inputs["tm_table"])
    run_sharded.write_diversity(out_dir, **inputs["diversity"])
    run_sharded.write_diversity_aligned(out_dir, **inputs["diversity_aligned"])
    run_sharded.write_tm_align_table(out_dir, **inputs["tm_align_table"])
    run_sharded.write_seq_diversity(out_dir, **inputs["seq_diversity"])


def test_writers_reproduce_their_files_byte_for_byte(tmp_path):
    write_all(str(tmp_path))
    want = sorted(os.listdir(GOLDEN))
    assert sorted(os.listdir(tmp_path)) == want and len(want) == 15
    for name in want:
        with open(os.path.join(GOLDEN, name), "rb") as f, open(tmp_path / name, "rb") as g:
            assert g.read() == f.read(), name


# ---- the stage plan of main() -----------------------------------------------------------------------------------------------------

# (command line, stage) in the order main() runs the stages; the values below are read off main() as it was with one block per flag
FLAGS = [(["--select"], "select"), (["--evaluate"], "evaluate"), (["--violations"], "violations"), (["--secondary-structure"], "secondary_structure"),
         (["--sasa"], "sasa"), (["--tm-score"], "tm_score"), (["--tm-align"], "tm_align"), (["--lddt"], "lddt"), (["--gdt"], "gdt"),
         (["--download-dir", "d", "--interface"], "interface"), (["--novelty", "set.npz"], "novelty"), (["--design"], "design")]
NEEDS_GROUND_TRUTH = {"evaluate", "sasa", "tm_score", "lddt", "gdt", "interface"}
SCORES_THE_SELECTION = {"evaluate", "lddt", "gdt", "interface"}


def test_stage_plan_truth_table():
    parse, plan_of = run_sharded.parse_args, run_sharded.stage_plan
    for inp in (False, True):
        none = plan_of(parse(["--out-dir", "x"]), inp)
        assert none.stages == () and not none.collect and not none.ground_truth and not none.keep_selection
    for argv, stage in FLAGS:
        for inp in (False, True):
            plan = plan_of(parse(["--out-dir", "x"] + argv), inp)
            assert [s.flag for s in plan.stages] == [stage] and plan.collect is True, argv
            assert plan.ground_truth is (inp and stage in NEEDS_GROUND_TRUTH) and plan.keep_selection is False, argv
            with_select = plan_of(parse(["--out-dir", "x", "--select"] + argv), inp)
            assert with_select.keep_selection is (stage in SCORES_THE_SELECTION), argv
            assert [s.flag for s in with_select.stages] == (["select"] if stage == "select" else ["select", stage])
    everything = parse(["--out-dir", "x", "--seq-diversity"] + [word for argv, stage in FLAGS if stage != "interface" for word in argv])
    everything.interface = True  # (the command line refuses --interface next to --novelty: the order of all rows is read off a namespace)
    plan = plan_of(everything, True)
    assert [s.flag for s in plan.stages] == [stage for _, stage in FLAGS] + ["seq_diversity"] == [s.flag for s in run_sharded.STAGES]
    assert plan.collect and plan.ground_truth and plan.keep_selection and not plan_of(everything, False).ground_truth
    design = plan_of(parse(["--out-dir", "x", "--design", "--seq-diversity", "--seq-align-mode", "local"]), False)
    assert [s.flag for s in design.stages] == ["design", "seq_diversity"] and design.collect and not design.ground_truth


def test_parse_args_refuses_what_main_refused(capsys):
    for argv, message in ((["--interface"], "de novo run has none"), (["--novelty", "s.npz", "--download-dir", "d"], "--novelty is for de novo runs"),
                          (["--seq-diversity"], "it needs --design"), (["--novelty-accuracy"], "needs --novelty SET.npz"), (["--keep", "some"], "expected all, last or an integer stride"),
                          (["--seq-align-mode", "local"], "the mode of --seq-diversity"), (["--novelty", "s.npz", "--novelty-top-k", "65"], "expected 1 .. 64")):
        with pytest.raises(SystemExit) as done:
            run_sharded.parse_args(["--out-dir", "x"] + argv)
        assert done.value.code == 2 and message in " ".join(capsys.readouterr().err.split()), argv
    assert run_sharded.parse_args(["--out-dir", "x", "--keep", "4"]).keep == 4 and run_sharded.parse_args(["--out-dir", "x"]).keep == "all"


# ---- the batch helpers ------------------------------------------------------------------------------------------------------------

def gathered_entries():
    """Two structures, "a" of 5 and "b" of 7 rows, two samples each (items 0, 1 and 2, 3).  Item 1 has none of the optional keys, item 2
    carries the ground truth of "b"."""
    rng = np.random.default_rng(5)
    records, gathered = [], {}
    for item, (name, sample_i, n) in enumerate((("a", 0, 5), ("a", 1, 5), ("b", 0, 7), ("b", 1, 7))):
        records.append({"item": item, "name": name, "sample_i": sample_i, "n_res": n, "rank": 0, "file": f"sample_{item:06d}.npz"})
        gathered[item] = {"prot": rng.standard_normal((n, 37, 3)).astype(np.float32), "diffused": np.arange(n) % 2 == 1,
                          "res_mask": np.r_[np.ones(n - 1, np.float32), np.float32(0)], "chain_idx": np.r_[np.ones(2), np.full(n - 2, 2.0)].astype(np.float32),
                          "aatype": np.arange(n, dtype=np.float32) + np.float32(0.25), "residue_index": np.arange(n)}
    for k in ("res_mask", "chain_idx", "aatype"):
        del gathered[1][k]
    gathered[2]["gt"] = rng.standard_normal((7, 37, 3)).astype(np.float32)
    return records, gathered


def test_padded_batch_shapes_dtypes_defaults_and_padding():
    records, gathered = gathered_entries()
    entries = [(gathered[i]["prot"], gathered[i]) for i in (0, 1, 2)]
    prot, diffused, res_mask, chain, aatype = run_sharded.padded_batch(entries, diffused=np.float32, res_mask=np.float32, chain_idx=np.int32, aatype=np.int64)
    assert prot.shape == (3, 7, 37, 3) and prot.dtype == np.float32
    assert [x.shape for x in (diffused, res_mask, chain, aatype)] == [(3, 7)] * 4
    assert [x.dtype for x in (diffused, res_mask, chain, aatype)] == [np.float32, np.float32, np.int32, np.int64]
    for b, i in enumerate((0, 1, 2)):
        n = gathered[i]["prot"].shape[0]
        assert np.array_equal(prot[b, :n], gathered[i]["prot"]) and not prot[b, n:].any()
        assert np.array_equal(diffused[b, :n], gathered[i]["diffused"].astype(np.float32))
        assert not any(x[b, n:].any() for x in (diffused, res_mask, chain, aatype))  # the padding: rows that do not exist
    assert res_mask[0].tolist() == [1, 1, 1, 1, 0, 0, 0] and res_mask[1].tolist() == [1, 1, 1, 1, 1, 0, 0] and res_mask[2].tolist() == [1, 1, 1, 1, 1, 1, 0]
    assert chain[0].tolist() == [1, 1, 2, 2, 2, 0, 0] and not chain[1].any() and chain[2].tolist() == [1, 1, 2, 2, 2, 2, 2]
    assert aatype[0].tolist() == [0, 1, 2, 3, 4, 0, 0] and not aatype[1].any()  # (rounded: 0.25 above an integer)
    only, int32 = run_sharded.padded_batch(entries[:2], aatype=np.int32)  # one key, another dtype; the longest of THESE entries
    assert only.shape == (2, 5, 37, 3) and int32.dtype == np.int32 and int32.shape == (2, 5)
    assert run_sharded.padded_batch([(gathered[2]["gt"], gathered[2])])[0].shape == (1, 7, 37, 3)  # a structure other than the entry's own


def test_row_masks_and_length_groups():
    records, gathered = gathered_entries()
    assert run_sharded.rows_that_exist(gathered[0]).tolist() == [1, 1, 1, 1, 0] and run_sharded.rows_that_exist(gathered[1]).tolist() == [1] * 5
    assert run_sharded.diffused_rows_that_exist(gathered[0]).tolist() == [0, 1, 0, 1, 0] and run_sharded.diffused_rows_that_exist(gathered[1]).tolist() == [0, 1, 0, 1, 0]
    assert run_sharded.diffused_rows_that_exist(gathered[2]).tolist() == [0, 1, 0, 1, 0, 1, 0]
    assert all(run_sharded.rows_that_exist(gathered[i]).dtype == np.float32 and run_sharded.diffused_rows_that_exist(gathered[i]).dtype == np.float32 for i in gathered)
    out_of_order = [records[3], records[0], records[2], records[1]]
    by_length = run_sharded.records_by_length(out_of_order, gathered)
    assert list(by_length) == [7, 5] and [[r["item"] for r in rs] for rs in by_length.values()] == [[3, 2], [0, 1]]  # first seen first
    assert list(run_sharded.records_by_length(records, gathered)) == [5, 7]
    prot, mask = run_sharded.stack_group(by_length[5], gathered)
    assert prot.shape == (2, 5, 37, 3) and prot.dtype == np.float32 and mask.dtype == np.float32
    assert np.array_equal(prot[1], gathered[1]["prot"]) and mask.tolist() == [[1, 1, 1, 1, 0], [1, 1, 1, 1, 1]]


def test_structures_by_name_appends_the_selected_structures():
    from framedipt_amd import selection
    records, gathered = gathered_entries()
    plain = list(run_sharded.structures_by_name(records[::-1], gathered))
    assert [(st.g, st.name, [r["item"] for r in st.records], st.labels) for st in plain] == [(0, "a", [0, 1], ["0", "1"]), (1, "b", [2, 3], ["0", "1"])]
    assert plain[0].truth is None and plain[1].truth is gathered[2]["gt"]
    assert all(x is gathered[i] for st in plain for x, i in zip(st.items, (r["item"] for r in st.records)))
    assert all(st.sources == st.items and all(s is it["prot"] for s, it in zip(st.structures, st.items)) for st in plain)
    # a selection by hand: per group the member each strategy builds on and, for mean / median, backbone columns of the diffused rows
    prot = run_sharded.padded_batch([(gathered[i]["prot"], gathered[i]) for i in range(4)])[0]
    sel = {"members": [np.array([0, 1]), np.array([2, 3])], "residues": [np.array([1, 3]), np.array([1, 3, 5])],
           "mean": [np.full((2, 4, 3), 7.0, np.float32), np.full((3, 4, 3), 8.0, np.float32)], "median": [np.full((2, 4, 3), 9.0, np.float32), np.full((3, 4, 3), 10.0, np.float32)],
           **{k: np.array([1, 0]) for k in ("mode", "mean_closest", "median_closest")}}
    for st in run_sharded.structures_by_name(records, gathered, {"selection": sel, "prot": prot}):
        n, s = st.items[0]["prot"].shape[0], len(st.records)
        assert st.labels == ["0", "1"] + list(selection.STRATEGIES) and len(st.structures) == len(st.sources) == s + len(selection.STRATEGIES)
        assert all(src is st.items[0] for src in st.sources[s:]) and st.sources[:s] == st.items
        for strategy, got in zip(selection.STRATEGIES, st.structures[s:]):
            assert got.shape == (n, 37, 3) and np.array_equal(got, selection.selected_structure(sel, st.g, strategy, prot)[:n])
