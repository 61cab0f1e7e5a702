"""GPU parity tests (-m gpu) of the merged IPA projection's point epilogue (csrc/ipa_proj2.hip: p2_points_walk, p2_node_rows): the
projection writes the rotated query / key / value points (qp, kpf, vpt, rot) and the node-row images (Kb, Vt, Vt_lo) itself, against
FDIPT_KF_POINTS_LAUNCH (the same projection on the unregrouped image, then points16_kernel: the path of the parent revision).  The point
columns are the same sums (same k order, same three products), rotated by the same expressions; the node-row images are the
projection's activation fragments, the conversions of fd_node_images."""
import numpy as np
import pytest

from conftest import kabsch_free_rmsd, load_golden
from test_gpu_round6 import _forward

pytestmark = pytest.mark.gpu


def _compare(a, b):
    rels = []
    for blk in range(1, 5):
        rel = np.linalg.norm(a["trace_node"][blk] - b["trace_node"][blk]) / np.linalg.norm(b["trace_node"][blk])
        rels.append(float(rel))
    dca = float(np.abs(a["rigids"][..., 4:] - b["rigids"][..., 4:]).max())
    return rels, dca


# N = 300: 20 padded keys (Np = 320); N = 40 (inpainting inputs): 24 padded keys; N = 64: none.  Not bit-identical (measured: node rows
# 9e-7 ... 2.3e-5 relative per block, frames 1.3e-5 ... 3.2e-5 A at N = 300 / 40): the rotation and the point columns are compiled
# into another kernel, whose floating-point contractions differ
@pytest.mark.parametrize("name", ["fwd_full_denovo_n300_t50", "fwd_full_inpaint_n40", "fwd_full_denovo_n64"])
def test_point_epilogue_against_the_point_launch(name):
    from framedipt_amd import _lib
    G = load_golden(name + ".npz")
    a, b = _forward(G, 0, trace=True), _forward(G, _lib.KF_POINTS_LAUNCH, trace=True)
    rels, dca = _compare(a, b)
    same = all(np.array_equal(a[k], b[k]) for k in a)
    print(f"{name}: point epilogue vs point launch: bit-identical {same}, node rel per block [{' '.join(f'{r:.1e}' for r in rels)}], "
          f"frames max {dca:.2e} A")
    # tolerances of the path comparison in test_gpu_round6.py
    for blk, rel in enumerate(rels, 1):
        assert rel < 5e-5, (blk, rel)
    assert dca < 1e-4
    if "denovo" in name:  # (the inpainting golden belongs to the inpainting network: test_gpu_parity.py)
        for o in (a, b):
            assert kabsch_free_rmsd(o["atom37"], G["out_atom37"]) < 5e-4


def test_outside_the_predicate_the_flag_changes_nothing():
    """The reference's formulation (FDIPT_KF_NO_MERGE) is outside the point epilogue's predicate: with and without
    FDIPT_KF_POINTS_LAUNCH the same kernels run, so every output is bit-identical."""
    from framedipt_amd import _lib
    G = load_golden("fwd_full_denovo_n300_t50.npz")
    a = _forward(G, _lib.KF_NO_MERGE, trace=True)
    b = _forward(G, _lib.KF_NO_MERGE | _lib.KF_POINTS_LAUNCH, trace=True)
    for k in a:
        assert np.array_equal(a[k], b[k]), k
