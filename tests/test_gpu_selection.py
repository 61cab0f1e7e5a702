"""GPU tests (-m gpu) of sample selection (framedipt_amd/selection.py -> fdipt_sample_select, csrc/select.hip) against the reference
fixture tests/golden/selection_cases.npz: every case as a group of its own and all cases as the groups of one launch."""
import functools

import numpy as np
import pytest
import torch

import selection_ref as sr
from conftest import load_golden

pytestmark = pytest.mark.gpu

# |device coordinate - reference| <= COORD_FACTOR x the reference's own spread under a permutation of its samples
# (selection_ref.coordinate_bound): the Gram sums, the matrix-vector product and the final combination run in another order
COORD_FACTOR = 32.0
PER_SAMPLE = ("weights", "density", "dist_to_mean", "dist_to_median")


@functools.lru_cache(maxsize=None)
def _fix():
    return load_golden("selection_cases.npz")


@functools.lru_cache(maxsize=None)
def _single(name):
    """One case as a launch of its own (NumPy inputs, uploaded)."""
    from framedipt_amd import selection
    prot, mask = sr.case_inputs(_fix(), name)
    return selection.select_samples(prot, mask)


@functools.lru_cache(maxsize=None)
def _joint():
    from framedipt_amd import selection
    prot, mask, groups = sr.joint_batch(_fix())
    assert prot.shape[1] % 4 != 0
    return selection.select_samples(prot, mask, groups)


@pytest.mark.parametrize("name", sr.CASES)
def test_case_matches_the_reference(name):
    """Indices exactly; mean and median within COORD_FACTOR x perm_diff; weights sum to 1 within 1e-12; densities to 1e-12 relative (the
    argument of exp is a sum of M <= 480 squares); the two distance vectors to 1e-12 relative against the restatement on the device's
    own reference points.  The single-sample case: the sample itself, status bit set, everything finite."""
    fix, got = _fix(), _single(name)
    prot, mask = sr.case_inputs(fix, name)
    x = sr.gather(prot, np.nonzero(mask[0])[0])
    bound = sr.coordinate_bound(fix, name, COORD_FACTOR)
    assert np.array_equal(got["residues"][0], np.nonzero(mask[0])[0]) and got["members"][0].tolist() == list(range(x.shape[0]))
    err_mean = np.abs(got["mean"][0] - fix[f"{name}.mean"]).max()
    print(f"{name}: |mean - ref| = {err_mean:.3e}, bound {bound:.3e}")
    assert err_mean <= bound
    assert abs(got["weights"][0].sum() - 1.0) <= 1e-12
    np.testing.assert_allclose(got["density"][0], fix[f"{name}.density"], rtol=1e-12)
    assert got["mode"][0] == int(fix[f"{name}.mode"]) and got["mean_closest"][0] == int(fix[f"{name}.mean_closest"])
    np.testing.assert_allclose(got["dist_to_mean"][0], sr.closest_distances(x, got["mean"][0]), rtol=1e-12)
    np.testing.assert_allclose(got["dist_to_median"][0], sr.closest_distances(x, got["median"][0]), rtol=1e-12, atol=1e-300)
    for k in PER_SAMPLE + ("mean", "median"):
        assert np.isfinite(got[k][0]).all(), k
    if x.shape[0] == 1:
        from framedipt_amd import selection
        assert got["status"][0] == selection.ZERO_DISTANCE and got["weights"][0].tolist() == [1.0]
        assert np.array_equal(got["median"][0], x[0]) and np.array_equal(got["mean"][0], x[0]) and got["median_closest"][0] == 0
        return
    err_median = np.abs(got["median"][0] - fix[f"{name}.median"]).max()
    print(f"{name}: |median - ref| = {err_median:.3e}, bound {bound:.3e}, perm_diff {float(fix[f'{name}.perm_diff']):.3e}")
    assert err_median <= bound
    assert got["status"][0] == 0 and got["median_closest"][0] == int(fix[f"{name}.median_closest"])
    # the weights are the median's: mu + sum_s w_s (x_s - mu)
    again = got["mean"][0] + np.tensordot(got["weights"][0], x - got["mean"][0][None], axes=1)
    assert np.abs(again - got["median"][0]).max() <= bound


def test_all_cases_in_one_launch_equal_their_own_launches():
    """Seven groups of mixed S (1 .. 64) and L (1 .. 40) in one launch, N not a multiple of 4, undiffused rows between and behind the
    regions: every group's outputs equal its single-group launch bit for bit."""
    joint = _joint()
    assert joint["group_ids"] == [100 + g for g in range(len(sr.CASES))]
    b = 0
    for g, name in enumerate(sr.CASES):
        one = _single(name)
        for k in PER_SAMPLE + ("mean", "median", "residues"):
            assert np.array_equal(joint[k][g], one[k][0]), (name, k)
        for k in ("mode", "mean_closest", "median_closest", "status"):
            assert joint[k][g] == one[k][0], (name, k)
        s = len(one["members"][0])
        assert joint["members"][g].tolist() == list(range(b, b + s))
        b += s


def test_device_tensor_and_numpy_array_agree():
    from framedipt_amd import selection
    prot, mask, groups = sr.joint_batch(_fix(), ("s5_two_chains", "s33_l9"))
    dev = selection.select_samples(torch.from_numpy(prot).cuda(), torch.from_numpy(mask).cuda(), groups)
    host = selection.select_samples(prot, mask, groups)
    for k in host:
        for a, b in zip(dev[k], host[k]):
            assert np.array_equal(a, b), k


def test_interleaved_groups_and_few_iterations():
    """Members of two groups interleaved in the batch (the member list, not the batch order, defines a group), and max_iterations = 0:
    the median is the mean, w = 1/S."""
    from framedipt_amd import selection
    fix = _fix()
    prot, mask = sr.case_inputs(fix, "s5_outlier")
    order = np.array([0, 4, 2, 1, 3])
    both = np.concatenate([prot, prot[order]])[[0, 5, 1, 6, 2, 7, 3, 8, 4, 9]]
    got = selection.select_samples(both, np.tile(mask[:1], (10, 1)), [0, 1] * 5)
    one = _single("s5_outlier")
    for k in PER_SAMPLE + ("mean", "median"):
        assert np.array_equal(got[k][0], one[k][0]), k
    assert got["members"][1].tolist() == [1, 3, 5, 7, 9] and got["mode"][1] == order.tolist().index(int(one["mode"][0]))
    zero = selection.select_samples(prot, mask, max_iterations=0)
    assert np.array_equal(zero["weights"][0], np.full(5, 0.2)) and np.abs(zero["median"][0] - zero["mean"][0]).max() <= 1e-13


def test_a_group_of_65_raises():
    from framedipt_amd import selection
    prot = torch.zeros(65, 8, 37, 3, device="cuda")
    with pytest.raises(ValueError, match="at most 64"):
        selection.select_samples(prot, torch.ones(65, 8, device="cuda"))


def test_end_to_end_inpainting_small_config():
    """Five inpainting samples of one structure (small config, N = 24, T = 3) in one batch, the result left on the device: selection on
    the device tensor equals selection on its host copy, and the ``median`` structure differs from member 0 in columns C, N, CA, O of
    the diffused residues only."""
    from framedipt_amd import config, inference, selection
    from framedipt_amd.diffusion import SE3Diffuser
    from framedipt_amd.model import ScoreNetwork
    from framedipt_amd.sampler import ConditionalSampler
    n, b = 24, 5
    conf = config.small_config(True)
    d = SE3Diffuser(conf.diffuser)
    net = ScoreNetwork(conf.model, d, inpainting=True, precision="fp32").load_synthetic(5).to("cuda")
    rng = np.random.default_rng(n)
    q = rng.standard_normal((n, 4))
    q /= np.linalg.norm(q, axis=-1, keepdims=True)
    tr = np.cumsum(rng.standard_normal((n, 3)) * 2.0, 0) + 30.0
    dm = np.zeros(n)
    dm[5:11], dm[16:19] = 1, 1
    feats_np = {"rigids_0": np.concatenate([q, tr], -1).astype(np.float32), "diffuse_mask": dm, "aatype": rng.integers(0, 20, n),
                "seq_idx": np.concatenate([np.arange(12), np.arange(12) + 212]), "chain_idx": np.repeat([0.0, 1.0], 12),
                "torsion_angles_sin_cos": np.tile(np.array([0.0, 1.0]), (n, 7, 1))}
    ds = ConditionalSampler.from_features([("synthetic", feats_np)], d, "cuda", samples=b)
    np.random.seed(3)
    items = [ds[i][2] for i in range(b)]
    feats = {k: torch.cat([it[k] for it in items], 0) for k in items[0]}
    res = inference.inference_fn(net, d, feats, num_t=3, min_t=0.01, aux_traj=True, noise_scale=0.1, inpainting=True, return_device=True)
    prot = res["prot_traj"][0]
    assert prot.is_cuda and tuple(prot.shape) == (b, n, 37, 3)
    diffuse = (1 - feats["fixed_mask"]) * feats["res_mask"]
    on_device = selection.select_samples(prot, diffuse)
    on_host = selection.select_samples(prot.cpu().numpy(), diffuse.cpu().numpy())
    for k in on_host:
        for a, c in zip(on_device[k], on_host[k]):
            assert np.array_equal(a, c), k
    assert on_device["residues"][0].tolist() == list(range(5, 11)) + list(range(16, 19)) and on_device["status"][0] == 0
    want = sr.select(sr.gather(prot.cpu().numpy(), on_device["residues"][0]))
    assert np.abs(on_device["median"][0] - want["median"]).max() <= sr.coordinate_bound(_fix(), "s1_l4", COORD_FACTOR)
    median = selection.selected_structure(on_device, 0, "median", prot)
    first = prot[0].cpu().numpy()
    changed = np.zeros((n, 37), dtype=bool)
    changed[np.ix_(on_device["residues"][0], [2, 0, 1, 4])] = True
    assert np.array_equal(median[~changed], first[~changed]) and (median[changed] != first[changed]).any()
    assert np.array_equal(median[on_device["residues"][0]][:, [2, 0, 1, 4]], on_device["median"][0].astype(np.float32))
    assert np.array_equal(selection.selected_structure(on_device, 0, "mode", prot), prot[int(on_device["mode"][0])].cpu().numpy())
