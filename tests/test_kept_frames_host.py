"""CPU tests of the kept-frame trajectories (``keep=``): the one rule that says which reverse steps keep their frames, and the ABI the
device side of it added (struct fields, the kept backbone entry) as the header, the binding derived from it and the built library state it."""
import os
import re

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_kept_steps_rule():
    """'all', 'last', stride 1, a stride that does not divide num_t - 1, a stride beyond num_t: ascending step indices, the final step
    always among them, and exactly the steps with (num_t - 1 - k) % s == 0."""
    from framedipt_amd.inference import kept_steps
    np.testing.assert_array_equal(kept_steps(20, "all"), np.arange(20))
    np.testing.assert_array_equal(kept_steps(20, "last"), [19])
    np.testing.assert_array_equal(kept_steps(20, 1), np.arange(20))
    np.testing.assert_array_equal(kept_steps(20, 3), [1, 4, 7, 10, 13, 16, 19])   # 19 = 6 * 3 + 1: the first step is not kept
    np.testing.assert_array_equal(kept_steps(20, 7), [5, 12, 19])
    np.testing.assert_array_equal(kept_steps(20, 19), [0, 19])
    np.testing.assert_array_equal(kept_steps(5, 7), [4])                          # s > num_t: the final step alone
    np.testing.assert_array_equal(kept_steps(1, "last"), [0])
    np.testing.assert_array_equal(kept_steps(1, 4), [0])
    np.testing.assert_array_equal(kept_steps(20, np.int64(3)), kept_steps(20, 3))
    for num_t in (1, 2, 5, 20, 101):
        for keep in ("all", "last", 1, 2, 3, 7, num_t, num_t + 3):
            k = kept_steps(num_t, keep)
            assert k.ndim == 1 and k[-1] == num_t - 1 and np.all(np.diff(k) > 0) and k[0] >= 0, (num_t, keep)
            if not isinstance(keep, str):
                np.testing.assert_array_equal(k, [i for i in range(num_t) if (num_t - 1 - i) % keep == 0])
                # the contract with the full trajectory: flipped, the kept steps are every keep-th row from row 0
                np.testing.assert_array_equal(k[::-1], np.arange(num_t)[::-1][::keep])


@pytest.mark.parametrize("bad", [0, -1, -3, 2.0, 1.5, "first", "", "3", None, True, False, (3,), [1]])
def test_kept_steps_refuses_bad_values(bad):
    from framedipt_amd.inference import kept_steps
    with pytest.raises(ValueError):
        kept_steps(20, bad)


def test_kept_steps_refuses_an_empty_trajectory():
    from framedipt_amd.inference import kept_steps
    with pytest.raises(ValueError):
        kept_steps(0, "last")


@pytest.mark.parametrize("struct,mirror", [("FdiptForwardArgs", "ForwardArgs"), ("FdiptReverseIndexed", "ReverseIndexed")])
def test_struct_mirrors_match_the_header(struct, mirror):
    """The two structs that carry the row map, as _lib derives them from include/fdipt.h (tests/test_abi_host.py holds them against the
    C layout): the new members sit directly behind step_cursor, at the end, and are zero (NULL / 0) by default."""
    from framedipt_amd import _lib
    cls = getattr(_lib, mirror)
    names = [n for n, _ in cls._fields_]
    new = {"FdiptForwardArgs": ["frame_rows", "state_ring"], "FdiptReverseIndexed": ["frame_rows", "state_ring", "kept_rigids"]}[struct]
    assert names[-len(new) - 1:] == ["step_cursor"] + new
    zero = cls()
    for n in new:
        assert not getattr(zero, n), n


def test_library_exports_the_kept_backbone_entry():
    """fdipt_backbone_atoms_kept: declared in the header beside fdipt_backbone_atoms_indexed (whose signature stays), bound by _lib and
    exported by the built library; it refuses a missing row map."""
    from framedipt_amd import _lib
    text = open(os.path.join(ROOT, "include", "fdipt.h")).read()
    assert re.search(r"int fdipt_backbone_atoms_kept\(int n, const float\* t7, const float\* psi, const int32_t\* aatype, const void\* tables,"
                     r"\s*float\* atom37_rows, const int32_t\* step_cursor, const int32_t\* frame_rows, fdipt_stream_t s\);", text)
    assert re.search(r"int fdipt_backbone_atoms_indexed\(int n, const float\* t7, const float\* psi, const int32_t\* aatype, const void\* tables,"
                     r"\s*float\* atom37_rows, const int32_t\* step_cursor, fdipt_stream_t s\);", text)
    assert len(_lib.SIGNATURES["fdipt_backbone_atoms_kept"][1]) == len(_lib.SIGNATURES["fdipt_backbone_atoms_indexed"][1]) + 1
    lib = _lib.load()
    assert lib.fdipt_backbone_atoms_kept(0, None, None, None, None, None, None, None, None) == 0      # n = 0: nothing to do
    assert lib.fdipt_backbone_atoms_kept(4, None, None, None, None, None, None, None, None) == -1     # FDIPT_EINVAL, no launch
    assert lib.fdipt_se3_reverse_step_indexed(None, None) == -1
