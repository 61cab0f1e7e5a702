"""Device noise on the host side (no GPU): known answers and distribution of the NumPy restatement the GPU tests measure the device code
against (tests/noise_ref.py), and the host plumbing that carries noise keys to the right samples."""
import numpy as np
import pytest
import torch

import noise_ref


@pytest.mark.parametrize("counter, key, words", [
    ((0, 0, 0, 0), (0, 0), "6627e8d5 e169c58d bc57ac4c 9b00dbd8"),
    ((0xffffffff,) * 4, (0xffffffff,) * 2, "408f276d 41c83b0e a20bc7c6 6d5451fd"),
    ((0x243f6a88, 0x85a308d3, 0x13198a2e, 0x03707344), (0xa4093822, 0x299f31d0), "d16cfe09 94fdcceb 5001e420 24126ea1"),
])
def test_philox_known_answers(counter, key, words):
    """The Random123 known-answer vectors of Philox4x32-10."""
    out = noise_ref.philox4x32_10(counter, key[0] | (key[1] << 32))
    assert " ".join(f"{int(w):08x}" for w in out) == words


def test_uniform_is_inside_the_open_interval():
    lo = noise_ref.uniform53(np.uint64(0), np.uint64(0))
    hi = noise_ref.uniform53(np.uint64(0xffffffff), np.uint64(0xffffffff))
    assert lo == 2.0 ** -54 and hi == 1.0 - 2.0 ** -54
    assert np.sqrt(-2 * np.log(lo)) < 8.7  # |z| < 8.7: what the GPU test's bound on device-minus-restatement rests on


def test_restatement_meets_the_distribution_bounds():
    """The keys, shapes and step counts of the GPU distribution test, on the restatement alone: it stays inside every bound, so a GPU
    failure means the device code and not an unlucky key."""
    T, N = noise_ref.DIST_T, noise_ref.DIST_N
    z = {p: noise_ref.normals(noise_ref.DIST_KEYS, p, 0, T, N) for p in range(4)}
    for p in range(4):
        bit = noise_ref.normals(noise_ref.DIST_BIT_KEYS, p, 0, T, N)
        for name, value, bound in noise_ref.distribution_report(z[p], z[p ^ 1], bit):
            print(f"purpose {p} {name}: {value:.3e} (bound {bound:.3e})")
            assert value < bound, (p, name, value, bound)


# ---------------------------------------------------------------------------------------------------------------------- host plumbing
class _Dataset:
    """Stands in for a sampler: items of different lengths whose x_T comes from the global np.random stream."""
    lengths = (62, 64, 61, 64, 300, 63)

    def __len__(self):
        return len(self.lengths)

    def __getitem__(self, item):
        n = self.lengths[item]
        rig = torch.zeros(1, n, 7)
        rig[..., 0] = 1
        rig[..., 4:] = torch.as_tensor(np.random.normal(size=(1, n, 3)), dtype=torch.float32)
        feats = {"rigids_t": rig, "res_mask": torch.ones(1, n), "fixed_mask": torch.zeros(1, n),
                 "seq_idx": torch.arange(1, n + 1)[None], "sc_ca_t": torch.zeros(1, n, 3)}
        return n, item % 2, feats


def test_seeded_item_returns_the_key_and_the_same_x_t():
    from framedipt_amd import sharding
    ds, seed = _Dataset(), 123
    for item in range(len(ds)):
        host = sharding.seeded_item(ds, item, seed, _Diffuser(), 10, 0.01)
        dev = sharding.seeded_item(ds, item, seed, None, 10, 0.01, noise="device")
        assert dev[3] == seed + item and isinstance(dev[3], int)
        assert isinstance(host[3], tuple) and host[3][0].shape == (9, 1, ds.lengths[item], 3)
        assert dev[:2] == host[:2] and torch.equal(dev[2]["rigids_t"], host[2]["rigids_t"])  # x_T: np.random.seed(seed + item) either way
    with pytest.raises(ValueError):
        sharding.seeded_item(ds, 0, seed, None, 10, 0.01, noise="gpu")


class _Diffuser:
    _diffuse_rot = _diffuse_trans = True


def test_mixed_batches_carry_keys_to_their_samples():
    from framedipt_amd import sharding
    ds, seed = _Dataset(), 40
    items = [sharding.seeded_item(ds, i, seed, None, 10, 0.01, noise="device") for i in range(len(ds))]
    groups = sharding.batches_mixed(list(ds.lengths), max_batch=4)
    assert sorted(p for g in groups for p in g) == list(range(len(ds))) and any(len(g) > 1 for g in groups)
    for g in groups:
        feats, keys, lengths = sharding.stack_items_padded([items[p] for p in g])
        assert keys.dtype == np.int64 and list(keys) == [seed + p for p in g]
        assert lengths == [ds.lengths[p] for p in g] and feats["rigids_t"].shape[:2] == (len(g), -(-max(lengths) // 4) * 4)
        for b, p in enumerate(g):  # the sample behind key b is item p
            assert torch.equal(feats["rigids_t"][b, :lengths[b]], items[p][2]["rigids_t"][0])
    feats, keys = sharding.stack_items([items[1], items[3]])
    assert list(keys) == [seed + 1, seed + 3] and feats["rigids_t"].shape[0] == 2
    f, k = sharding.pad_item(items[0][2], items[0][3], 64)
    assert k == seed and f["rigids_t"].shape[1] == 64


def test_noise_keys_argument():
    from framedipt_amd import noise
    assert list(noise.as_keys(7, 3)) == [7, 8, 9]
    assert list(noise.as_keys(torch.tensor([5, -1, 2 ** 63 - 1]), 3)) == [5, 2 ** 64 - 1, 2 ** 63 - 1]
    assert noise.as_keys([1, 2], 2).dtype == np.uint64
    with pytest.raises(ValueError):
        noise.as_keys([1, 2], 3)


def test_device_noise_argument_errors_come_before_any_device_work():
    """noise="device" with a tape, or without keys, is a ValueError raised ahead of everything else (no GPU here: a dummy model)."""
    from framedipt_amd import confidence, inference
    feats = {"rigids_t": torch.zeros(2, 8, 7)}
    tape = (np.zeros((3, 2, 8, 3)), np.zeros((3, 2, 8, 3)))
    for fn in (lambda **kw: inference.inference_fn(None, None, feats, num_t=4, min_t=0.01, **kw),
               lambda **kw: inference.ReverseLoop(None, None, feats, 4, 0.01, **kw),
               lambda **kw: inference.StreamedLoops(None, None, feats, 2, 4, 0.01, **kw)):
        with pytest.raises(ValueError, match="noise_tape"):
            fn(noise="device", noise_keys=3, noise_tape=tape)
        with pytest.raises(ValueError, match="noise_keys"):
            fn(noise="device")
        with pytest.raises(ValueError, match="noise_keys"):
            fn(noise="host", noise_keys=3)
        with pytest.raises(ValueError):
            fn(noise="device", noise_keys=[1, 2, 3])  # three keys for two samples
        with pytest.raises(ValueError):
            fn(noise="tape")


def test_run_sharded_takes_the_noise_flag():
    import inspect

    from framedipt_amd import run_sharded
    assert inspect.signature(run_sharded.run_rank).parameters["noise"].default == "host"
    assert run_sharded.parse_args(["--out-dir", "x"]).noise == "host"
    assert run_sharded.parse_args(["--out-dir", "x", "--noise", "device"]).noise == "device"
    with pytest.raises(SystemExit) as done:  # (a choice of host / device)
        run_sharded.parse_args(["--out-dir", "x", "--noise", "both"])
    assert done.value.code == 2
    assert '"noise": a.noise' in inspect.getsource(run_sharded.main)  # (the manifest's meta)
