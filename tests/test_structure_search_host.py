"""CPU tests of the novelty search's host side (framedipt_amd/structure_search.py): the packed structure set
and its readers, the work plan of the score pass, the length bound against the brute force (tests/search_ref.py) and the order rule."""
import gzip
import os

import numpy as np
import pytest

import search_ref as sr
from conftest import GOLDEN
from framedipt_amd import _lib, output, structure_search as ss
from framedipt_amd.data import features, mmcif

CAPS = ss.BUCKET_CAPS
STRUCTURES = os.path.join(GOLDEN, "search_structures")
# chain -> (rows of the feature builder, rows with a CA atom) of the three test complexes
CHAINS = {"1fyt": {"A": (198, 180), "B": (196, 179), "C": (14, 13), "D": (227, 198), "E": (277, 240)},
          "5ksa": {"A": (354, 183), "B": (332, 190), "C": (335, 195), "D": (409, 242), "J": (25, 11)},
          "7t2d": {"A": (182, 180), "B": (172, 171), "C": (15, 14), "D": (201, 201), "E": (238, 235), "U": (4, 0)}}


def _walk(rng, n):
    return np.cumsum(rng.normal(size=(n, 3)) * 2.2, axis=0).astype(np.float32)


# ------------------------------------------------------------------------------------------------------ StructureSet
def test_save_and_load_keep_the_bytes(tmp_path):
    rng = np.random.default_rng(3)
    db = ss.StructureSet.from_arrays([_walk(rng, n) for n in (7, 1, 0, 600)], names=["a", "b:A", "", "long one"])
    assert len(db) == 4 and db.lengths.tolist() == [7, 1, 0, 600] and db.offsets.dtype == np.int64 and db.ca.dtype == np.float32 and db.ca.shape == (608, 3)
    path = tmp_path / "set.npz"
    db.save(path)
    back = ss.StructureSet.load(path)
    assert back.ca.tobytes() == db.ca.tobytes() and back.offsets.tobytes() == db.offsets.tobytes() and back.names == db.names
    with np.load(path, allow_pickle=False) as z:  # arrays and names only
        assert sorted(z.files) == ["ca", "names", "offsets"]
    assert np.array_equal(back.entry(3), db.ca[8:]) and ss.StructureSet.from_arrays([np.zeros((3, 3))]).names == ["0"]
    with pytest.raises(ValueError, match="offsets"):
        ss.StructureSet(db.ca, [0, 7, 5, 608])
    with pytest.raises(ValueError, match="names"):
        ss.StructureSet(db.ca, db.offsets, ["a"])


def test_from_structures_drops_masked_rows_in_every_layout():
    rng = np.random.default_rng(4)
    ca = np.stack([_walk(rng, 12), _walk(rng, 12)])
    mask = np.ones((2, 12), dtype=np.float32)
    mask[0, [0, 5, 6]] = 0
    mask[1, 9:] = 0
    five = np.stack([sr.ta.five_atoms(c) for c in ca])
    wide = np.zeros((2, 12, 37, 3), dtype=np.float32)
    wide[:, :, :5] = five
    for prot in (ca, five, wide):
        db = ss.StructureSet.from_structures(prot, mask, names=["x", "y"])
        assert db.lengths.tolist() == [9, 9] and db.names == ["x", "y"]
        assert np.array_equal(db.entry(0), ca[0][mask[0] != 0]) and np.array_equal(db.entry(1), ca[1][:9])
    assert ss.StructureSet.from_structures(five).lengths.tolist() == [12, 12]
    with pytest.raises(ValueError, match="prot should be"):
        ss.StructureSet.from_structures(np.zeros((2, 12, 4, 3)))
    with pytest.raises(ValueError, match="mask"):
        ss.StructureSet.from_structures(five, np.ones((2, 11)))


def test_from_directory_gives_one_entry_per_chain_of_the_three_test_complexes(tmp_path):
    """The files are the reference's test complexes cut down to their CA atoms and HETATM records, kept compressed
    (tests/golden/make_goldens_search.py): the feature builder counts every residue, waters and ligands among them; the set keeps the
    rows with a CA atom."""
    for name in CHAINS:
        with gzip.open(os.path.join(STRUCTURES, f"{name}-assembly1.cif.gz"), "rb") as f:
            (tmp_path / f"{name}-assembly1.cif").write_bytes(f.read())
    db = ss.StructureSet.from_directory(tmp_path, "*.cif")
    want = [(f"{name}-assembly1.cif:{chain}", rows) for name, chains in CHAINS.items() for chain, (_, rows) in chains.items()]
    assert list(zip(db.names, db.lengths.tolist())) == want and len(db) == 16
    ca = features.ATOM_ORDER["CA"]
    e = 0
    for name, chains in CHAINS.items():
        rows, _ = mmcif.read_atom_site(tmp_path / f"{name}-assembly1.cif")
        built = mmcif.chain_features(rows)
        assert {c: (len(f["aatype"]), int(f["atom_mask"][:, ca].sum())) for c, f in built.items()} == chains
        for chain, f in built.items():
            assert np.array_equal(db.entry(e), f["atom_positions"][f["atom_mask"][:, ca] != 0, ca].astype(np.float32))
            e += 1
    assert len(ss.StructureSet.from_directory(tmp_path, "1fyt*")) == 5 and len(ss.StructureSet.from_directory(tmp_path, "*.pdb")) == 0


def test_from_directory_reads_pdb_files_and_drops_rows_without_a_ca(tmp_path):
    rng = np.random.default_rng(5)
    pos = np.zeros((9, 37, 3), dtype=np.float32)
    pos[:, :5] = sr.ta.five_atoms(_walk(rng, 9))
    output.write_prot_to_pdb(pos, str(tmp_path / "s.pdb"), overwrite=True, no_indexing=True)
    text = (tmp_path / "s.pdb").read_text().split("\n")
    text = [line[:21] + "B" + line[22:] if line.startswith("ATOM") and int(line[22:26]) >= 5 else line for line in text]  # a second chain
    third = [k for k, line in enumerate(text) if line.startswith("ATOM") and line[12:16].strip() == "CA"][2]
    del text[third]  # the third residue loses its CA
    (tmp_path / "s.pdb").write_text("\n".join(text))
    db = ss.StructureSet.from_directory(tmp_path, "*.pdb")
    assert [n.split(":")[0] for n in db.names] == ["s.pdb", "s.pdb"] and db.lengths.tolist() == [4, 4]
    kept = np.round(pos[[0, 1, 3, 4, 5, 6, 7, 8], 1], 3)
    assert np.abs(db.ca - kept).max() <= 1e-3  # (the file holds three decimals)


# ------------------------------------------------------------------------------------------------------ the planner
def test_every_entry_falls_into_the_smallest_cap_that_holds_it():
    lengths = np.arange(0, ss.MAX_ROWS + 40)
    got = ss.plan(lengths)
    for n, b, long in zip(lengths, got["bucket_of"], got["too_long"]):
        if n > ss.MAX_ROWS:
            assert long and b == -1
        else:
            assert not long and CAPS[b] >= n and (b == 0 or CAPS[b - 1] < n)
    assert sorted(got["entries"].tolist()) == list(range(ss.MAX_ROWS + 1)) and got["detail_cap"] == ss.MAX_ROWS
    assert list(CAPS) == sorted(set(CAPS)) and CAPS[-1] == ss.MAX_ROWS == _lib.TMA_MAX_ROWS


@pytest.mark.parametrize("rank_by", ["query", "target"])
def test_bucket_edges_the_row_limit_and_the_order_of_the_buckets(rank_by):
    lengths = [n for cap in CAPS for n in (cap - 1, cap, cap + 1)]
    assert lengths[-1] == 513
    got = ss.plan(lengths, rank_by)
    for k, cap in enumerate(CAPS):
        below, at, above = got["bucket_of"][3 * k:3 * k + 3]
        assert CAPS[below] == cap and CAPS[at] == cap and (above == -1 if cap == CAPS[-1] else CAPS[above] == CAPS[k + 1])
    assert got["too_long"].tolist() == [False] * (len(lengths) - 1) + [True] and 3 * len(CAPS) - 1 not in got["entries"]
    # the launches in order: the caps fall ("query") or rise ("target"), and so does the largest bound of a bucket for any query length
    caps = got["bucket_cap"].tolist()
    assert caps == sorted(CAPS, reverse=rank_by == "query") and got["bucket_start"][0] == 0 and got["bucket_start"][-1] == len(got["entries"])
    members = [got["entries"][s:e] for s, e in zip(got["bucket_start"][:-1], got["bucket_start"][1:])]
    for cap, m in zip(caps, members):
        assert (np.asarray(lengths)[m] <= cap).all() and m.tolist() == sorted(m.tolist())
    for n1 in (5, 60, 300, 512):
        best = [max(ss.bound(n1, np.asarray(lengths)[m], rank_by)) for m in members]
        assert all(a >= b for a, b in zip(best, best[1:])), (n1, best)
    with pytest.raises(ValueError, match="rank_by"):
        ss.plan(lengths, "length")


def test_a_set_of_entries_beyond_the_limit_plans_no_launch():
    got = ss.plan([513, 600])
    assert len(got["entries"]) == 0 and got["bucket_start"].tolist() == [0] and len(got["bucket_cap"]) == 0 and got["too_long"].all()


# ------------------------------------------------------------------------------------------------------ the bound, the order rule
def test_the_restatement_stays_at_or_below_the_length_bound_on_every_pair_of_the_gpu_cases():
    _, _, entries, _ = sr.case_a()
    ref = sr.case_a_ref(top_k=4)
    scored = 0
    for q, x in enumerate(sr.case_a_queries()):
        for e, y in enumerate(entries):
            if np.isnan(ref["scores_q"][q, e]):
                assert ref["pair_status"][q, e] != 0
                continue
            scored += 1
            assert ref["scores_q"][q, e] <= sr.bound(len(x), len(y), "query") == ss.bound(len(x), len(y), "query")
            assert ref["scores_t"][q, e] <= sr.bound(len(x), len(y), "target") == ss.bound(len(x), len(y), "target")
    assert scored == 3 * 14 and ss.bound(60, 60) == 1.0 and ss.bound(60, 59) < 1.0 and ss.bound(60, 130, "target") == 60 / 130


def test_search_ref_orders_ties_by_entry_index_and_applies_min_score_and_top_k():
    ref = sr.case_a_ref(top_k=4)
    row = ref["hit"][1].tolist()  # the 60-row query: its two copies tie bit for bit
    assert row.index(sr.SELF) + 1 == row.index(sr.DUPLICATE) and ref["scores_q"][1, sr.SELF] == ref["scores_q"][1, sr.DUPLICATE] == 1.0
    for q in range(3):
        s = ref["tm_q"][q]
        assert (np.diff(s) <= 0).all() and not np.isnan(s).any() and ref["pdb_tm"][q] == s[0]
    few = sr.case_a_ref(top_k=8, min_score=0.5)
    assert ((few["tm_q"] >= 0.5) == (few["hit"] >= 0)).all() and np.isnan(few["tm_q"][few["hit"] < 0]).all() and (few["hit"][2] == -1).all()
    by_target = sr.case_a_ref(top_k=2, rank_by="target")
    assert (np.diff(by_target["tm_t"], axis=1) <= 0).all() and (by_target["pdb_tm"] == by_target["tm_t"][:, 0]).all()


def test_search_refuses_bad_arguments_before_the_device_is_touched():
    prot, mask, entries, names = sr.case_a()
    db = ss.StructureSet.from_arrays(entries, names)
    with pytest.raises(ValueError, match="top_k"):
        ss.search(prot, db, mask, top_k=0)
    with pytest.raises(ValueError, match="top_k"):
        ss.search(prot, db, mask, top_k=ss.MAX_K + 1)
    with pytest.raises(ValueError, match="rank_by"):
        ss.search(prot, db, mask, rank_by="both")
    with pytest.raises(ValueError, match="empty"):
        ss.search(prot, ss.StructureSet.from_arrays([]), mask)
    with pytest.raises(ValueError, match="prot should be"):
        ss.search(prot[:, :, 1], db, mask)
    assert ss.MAX_K == 64 == _lib.SEARCH_MAX_K and ss.PRUNED == 16 and ss.TOO_LONG == 32
