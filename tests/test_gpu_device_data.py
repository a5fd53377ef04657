"""GPU: device-resident training batches -- geoadv_batch_gather (csrc/dataset.hip) through the C interface and ops.batch_gather,
device_data.DevicePointCloudDataSet against in_out.PointCloudDataSet, the augmentation / denoising paths of PointNetAETrainer
and the new flags of train_ae and train_classifier.

The noise is held to the float64 restatement of the generator on the same uniforms (tests/_batch_noise64.py) within
    |out - ref| <= sigma 2^-19 max(1, |g|) + 2^-23 (|x| + |mu| + sigma |g|).
Derived, not measured: a 1-ulp logf and sqrtf and a 2-ulp cospif leave g within 2^-21 relative on |g| <= 5.77 (the largest
value 24-bit uniforms can give), widened by 4 for freedom of implementation; the second term covers the three fp32 roundings of
sigma g, mu + . and x + . .  The rotation is held to numpy's float64 product rounded to fp32 within one fp32 ulp."""
import ctypes
import json
import os

import numpy as np
import pytest

import _batch_noise64 as BN

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
INDEX = [6, 0, 6, 3, 1]
EINVAL = 1


def _clouds(seed, b, n):
    return (np.random.default_rng(seed).random((b, n, 3)) - 0.5).astype(np.float32)


def _dev(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def _guarded(count, offset, pad=64, fill=None):
    """A NaN-filled allocation of count + 2 pad floats; -> (tensor, pointer to element `offset`)."""
    import torch
    t = torch.full((count + 2 * pad,), float("nan"), dtype=torch.float32, device=DEV)
    if fill is not None:
        t[offset:offset + count] = _dev(fill.reshape(-1))
    return t, ctypes.c_void_p(t.data_ptr() + 4 * offset)


def _guards_intact(t, count, offset):
    import torch
    return bool(torch.isnan(t[:offset]).all() and torch.isnan(t[offset + count:]).all())


def _aug(**kw):
    from geometric_adv_amd.ops import BatchAugment
    return BatchAugment(**kw)


def _raw(L, b, n, data_ptr, num_clouds, index, aug, rot, clean_ptr, feed_ptr):
    from geometric_adv_amd import _lib
    return L.geoadv_batch_gather(b, n, data_ptr, ctypes.c_longlong(num_clouds), _lib.ptr(index),
                                 ctypes.byref(aug) if aug is not None else None, _lib.ptr(rot), clean_ptr, feed_ptr,
                                 _lib.stream_handle())


# ---- gather ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("with_index", [True, False], ids=["index", "in_order"])
@pytest.mark.parametrize("n", [1, 63, 64, 65, 200])
def test_gather_is_bit_equal_inside_guards(n, with_index):
    """Straight through the C interface, every buffer inside a NaN-filled allocation: at a 16-byte aligned start (four points per
    thread where n % 4 == 0) and at an unaligned one (one point per thread).  clean and the un-augmented feed hold the bits of
    data[index]; no guard changes."""
    from geometric_adv_amd import _lib
    L = _lib.lib()
    data = _clouds(n, 7, n)
    b = 5
    want = data[INDEX] if with_index else data[:b]
    index = _dev(np.array(INDEX, np.int32)) if with_index else None
    for offset in (4, 5):
        src, src_p = _guarded(data.size, offset, fill=data)
        count = b * n * 3
        clean, clean_p = _guarded(count, offset)
        feed, feed_p = _guarded(count, offset)
        _lib.check(_raw(L, b, n, src_p, 7, index, None, None, clean_p, feed_p), "batch_gather")
        for name, t in (("clean", clean), ("feed", feed)):
            assert _guards_intact(t, count, offset), "%s: a guard changed (offset %d)" % (name, offset)
            got = t[offset:offset + count].cpu().numpy().reshape(b, n, 3)
            assert np.array_equal(_bits(got), _bits(want)), "%s differs (offset %d)" % (name, offset)
        assert _guards_intact(src, data.size, offset)
        # feed alone (clean == NULL), and a noise-free augment structure
        feed2, feed2_p = _guarded(count, offset)
        _lib.check(_raw(L, b, n, src_p, 7, index, _aug(seed=1, noise_mu=0.5), None, None, feed2_p), "batch_gather")
        assert _guards_intact(feed2, count, offset)
        assert np.array_equal(_bits(feed2[offset:offset + count].cpu().numpy().reshape(b, n, 3)), _bits(want))


def test_op_gathers_and_checks_host_indices():
    import torch
    from geometric_adv_amd import ops
    data = _clouds(1, 7, 65)
    x = _dev(data)
    clean, feed = ops.batch_gather(x, INDEX, want_clean=True)
    assert np.array_equal(_bits(clean.cpu().numpy()), _bits(data[INDEX])) and np.array_equal(_bits(feed.cpu().numpy()), _bits(data[INDEX]))
    assert np.array_equal(_bits(ops.batch_gather(x).cpu().numpy()), _bits(data))
    assert np.array_equal(_bits(ops.batch_gather(x, np.array(INDEX, np.int64)).cpu().numpy()), _bits(data[INDEX]))
    assert np.array_equal(_bits(ops.batch_gather(x, torch.tensor(INDEX, device=DEV)).cpu().numpy()), _bits(data[INDEX]))
    for bad in ([0, 7], [-1, 2], np.array([3, 1 << 40])):
        with pytest.raises(ValueError, match="out of range"):
            ops.batch_gather(x, bad)
    with pytest.raises(ValueError):
        ops.batch_gather(x, [[0, 1]])
    with pytest.raises(ValueError):
        ops.batch_gather(x, [0.0, 1.0])
    with pytest.raises(ValueError):
        ops.batch_gather(x, INDEX, rot=np.eye(3)[None].repeat(2, 0))
    with pytest.raises(ValueError):
        ops.batch_gather(torch.from_numpy(data), INDEX)


def test_a_device_index_out_of_range_is_never_dereferenced():
    """Only a device index can reach the kernel unchecked: its slot stays unwritten, the others are served."""
    from geometric_adv_amd import _lib
    L = _lib.lib()
    n, b = 65, 5
    data = _clouds(2, 7, n)
    src, src_p = _guarded(data.size, 4, fill=data)
    index = _dev(np.array([6, 7, -1, 0, 2 ** 31 - 1], np.int32))
    count = b * n * 3
    clean, clean_p = _guarded(count, 4)
    feed, feed_p = _guarded(count, 4)
    _lib.check(_raw(L, b, n, src_p, 7, index, _aug(seed=3, noise_sigma=0.01), None, clean_p, feed_p), "batch_gather")
    got_clean = clean[4:4 + count].cpu().numpy().reshape(b, n, 3)
    got_feed = feed[4:4 + count].cpu().numpy().reshape(b, n, 3)
    assert np.array_equal(_bits(got_clean[[0, 3]]), _bits(data[[6, 0]]))
    assert np.isnan(got_clean[[1, 2, 4]]).all() and np.isnan(got_feed[[1, 2, 4]]).all()
    assert np.isfinite(got_feed[[0, 3]]).all()
    assert _guards_intact(clean, count, 4) and _guards_intact(feed, count, 4)


# ---- noise -------------------------------------------------------------------------------------------------------------
NOISE_CASES = [(0.0, 0.05, 0.05), (0.0, 0.01, 0.05), (0.1, 0.02, None)]


@pytest.mark.parametrize("n", [65, 200])
@pytest.mark.parametrize("mu,sigma,clip", NOISE_CASES)
def test_noise_against_the_float64_restatement(mu, sigma, clip, n):
    from geometric_adv_amd import ops
    data = _clouds(3, 7, n)
    x = _dev(data)
    seed, counter = 7, 1
    aug = dict(seed=seed, counter=counter, noise_mu=mu, noise_sigma=sigma, noise_clip=clip or 0.0)
    clean, feed = ops.batch_gather(x, INDEX, aug, want_clean=True)
    got = feed.cpu().numpy()
    assert np.array_equal(_bits(clean.cpu().numpy()), _bits(data[INDEX]))
    g = BN.normals(seed, counter, np.arange(5), n)
    src = data[INDEX].astype(np.float64)
    ref = src + BN.noise(g, mu, sigma, clip)
    s32, m32 = float(np.float32(sigma)), float(np.float32(mu))
    bound = s32 * 2.0 ** -19 * np.maximum(1.0, np.abs(g)) + 2.0 ** -23 * (np.abs(src) + abs(m32) + s32 * np.abs(g))
    err = np.abs(got.astype(np.float64) - ref)
    print("largest error / bound: %.3f" % (err / bound).max())
    assert np.all(err <= bound)
    if clip is not None and sigma >= clip:
        clamped = np.mean(np.abs(s32 * g) > clip)
        assert 0.25 < clamped < 0.4, clamped                      # one sigma: about a third of the draws sit on the clamp
        assert np.abs(got.astype(np.float64) - src).max() <= clip + 2.0 ** -23
    # a repeated call is bit-equal; the same clouds twice in the batch (index 6) get different noise
    assert np.array_equal(_bits(ops.batch_gather(x, INDEX, aug).cpu().numpy()), _bits(got))
    assert not np.array_equal(got[0], got[2])
    # slots 2..4 on their own: what data-parallel rank 1 of a 2 + 3 split gathers
    part = ops.batch_gather(x, INDEX[2:], dict(aug, slot_offset=2)).cpu().numpy()
    assert np.array_equal(_bits(part), _bits(got[2:]))
    # another counter, another seed: other values (but for draws that sit on the same side of the clamp)
    assert np.mean(ops.batch_gather(x, INDEX, dict(aug, counter=counter + 1)).cpu().numpy() == got) < 0.2
    assert np.mean(ops.batch_gather(x, INDEX, dict(aug, seed=seed + 1)).cpu().numpy() == got) < 0.2


def test_sigma_zero_ignores_mu():
    from geometric_adv_amd import ops
    data = _clouds(4, 7, 64)
    got = ops.batch_gather(_dev(data), INDEX, dict(seed=7, noise_mu=0.1, noise_sigma=0.0)).cpu().numpy()
    assert np.array_equal(_bits(got), _bits(data[INDEX]))


# ---- rotation ----------------------------------------------------------------------------------------------------------
def _within_one_ulp(got, want):
    ulp = np.spacing(np.maximum(np.abs(got), np.abs(want)))
    return np.all(np.abs(got.astype(np.float64) - want.astype(np.float64)) <= ulp)


def _y_matrices(angles):
    return np.stack([np.array([[np.cos(a), 0.0, np.sin(a)], [0.0, 1.0, 0.0], [-np.sin(a), 0.0, np.cos(a)]]) for a in angles])


@pytest.mark.parametrize("n", [65, 200])
def test_rotation_against_numpy_float64(n):
    from geometric_adv_amd import ops
    from geometric_adv_amd.device_data import rand_rotation_matrix
    data = _clouds(5, 7, n)
    x = _dev(data)
    src = data[INDEX].astype(np.float64)
    R = rand_rotation_matrix(seed=4)
    got = ops.batch_gather(x, INDEX, rot=R).cpu().numpy()
    assert _within_one_ulp(got, (src @ R).astype(np.float32))
    Rs = _y_matrices([0.3, 1.1, 2.0, 3.5, 6.0])
    clean, got = ops.batch_gather(x, INDEX, rot=Rs, want_clean=True)
    assert _within_one_ulp(got.cpu().numpy(), np.einsum("bnk,bkj->bnj", src, Rs).astype(np.float32))
    assert np.array_equal(_bits(clean.cpu().numpy()), _bits(data[INDEX]))
    # the same matrices as a float64 GPU tensor
    assert np.array_equal(_bits(ops.batch_gather(x, INDEX, rot=_dev(Rs)).cpu().numpy()), _bits(got.cpu().numpy()))
    # copies and sign flips are exact
    assert np.array_equal(_bits(ops.batch_gather(x, INDEX, rot=np.eye(3)).cpu().numpy()), _bits(data[INDEX]))
    P = np.array([[0.0, -1.0, 0.0], [0.0, 0.0, 1.0], [1.0, 0.0, 0.0]])
    want = np.stack([data[INDEX][..., 2], -data[INDEX][..., 0], data[INDEX][..., 1]], axis=-1)
    assert np.array_equal(_bits(ops.batch_gather(x, INDEX, rot=P).cpu().numpy()), _bits(want))


@pytest.mark.parametrize("n", [65, 200])
def test_each_order_of_noise_and_rotation(n):
    """The noise belongs to (seed, counter, slot, point, coordinate) and not to the data, so each order is rebuilt bit for bit from
    two single-stage calls: rotate_first 0 = the rotation of the noisy clouds, rotate_first 1 = the noise on the rotated clouds."""
    from geometric_adv_amd import ops
    data = _clouds(6, 7, n)
    x = _dev(data)
    Rs = _y_matrices([0.3, 1.1, 2.0, 3.5, 6.0])
    noise = dict(seed=11, counter=2, noise_mu=0.01, noise_sigma=0.02)
    noisy = ops.batch_gather(x, INDEX, noise)
    rotated = ops.batch_gather(x, INDEX, rot=Rs)
    ae_order = ops.batch_gather(x, INDEX, dict(noise, rotate_first=0), rot=Rs).cpu().numpy()
    cls_order = ops.batch_gather(x, INDEX, dict(noise, rotate_first=1), rot=Rs).cpu().numpy()
    assert np.array_equal(_bits(ae_order), _bits(ops.batch_gather(noisy, None, rot=Rs).cpu().numpy()))
    assert np.array_equal(_bits(cls_order), _bits(ops.batch_gather(rotated, None, noise).cpu().numpy()))
    assert not np.array_equal(ae_order, cls_order)


# ---- refusals ----------------------------------------------------------------------------------------------------------
def test_refusals():
    import torch
    from geometric_adv_amd import _lib
    L = _lib.lib()
    b, n = 5, 64
    data = _dev(_clouds(7, 7, n))
    feed, clean = torch.empty((b, n, 3), device=DEV), torch.empty((b, n, 3), device=DEV)
    rot = _dev(np.eye(3)[None].repeat(5, 0))
    dp, fp, cp, null = _lib.ptr(data), _lib.ptr(feed), _lib.ptr(clean), ctypes.c_void_p(0)
    assert _raw(L, b, n, dp, 7, None, None, None, cp, fp) == 0
    assert _raw(L, 0, n, dp, 7, None, None, None, cp, fp) == EINVAL
    assert _raw(L, b, 0, dp, 7, None, None, None, cp, fp) == EINVAL
    assert _raw(L, b, n, dp, 0, None, None, None, cp, fp) == EINVAL
    assert _raw(L, b, n, dp, 7, None, _aug(rot_count=2), rot, cp, fp) == EINVAL
    assert _raw(L, b, n, dp, 7, None, _aug(rot_count=-1), rot, cp, fp) == EINVAL
    assert _raw(L, b, n, dp, 7, None, _aug(rot_count=1), None, cp, fp) == EINVAL
    assert _raw(L, b, n, dp, 7, None, _aug(rot_count=5), None, cp, fp) == EINVAL
    assert _raw(L, b, n, dp, 7, None, None, None, cp, null) == EINVAL
    assert _raw(L, b, n, null, 7, None, None, None, cp, fp) == EINVAL
    assert _raw(L, b, n, dp, 7, None, None, None, cp, dp) == EINVAL                       # feed is data
    assert _raw(L, b, n, dp, 7, None, None, None, dp, fp) == EINVAL                       # clean is data
    inside = ctypes.c_void_p(data.data_ptr() + 12 * n)                                    # ... or lies inside it
    assert _raw(L, b, n, dp, 7, None, None, None, null, inside) == EINVAL
    assert _raw(L, b, n, dp, 7, None, None, None, fp, fp) == EINVAL                       # clean is feed
    assert _raw(L, b, n, dp, 7, None, _aug(slot_offset=-1), None, cp, fp) == EINVAL
    assert _raw(L, b, n, dp, 7, None, _aug(noise_sigma=-0.5), None, cp, fp) == EINVAL
    assert b"sigma" in L.geoadv_last_error()
    assert _raw(L, b, n, dp, 7, None, _aug(rot_count=5, noise_sigma=0.01), rot, cp, fp) == 0


# ---- the data set ------------------------------------------------------------------------------------------------------
def test_device_set_serves_the_host_set_s_batches():
    from geometric_adv_amd.device_data import DevicePointCloudDataSet
    from geometric_adv_amd.in_out import PointCloudDataSet
    pcs, noisy = _clouds(8, 11, 64), _clouds(9, 11, 64)
    labels = np.array(["cloud_%02d" % i for i in range(11)], dtype=object)
    np.random.seed(3)
    host = PointCloudDataSet(pcs, noise=noisy, labels=labels)
    host_batches = [tuple(np.array(a) for a in host.next_batch(4)) + (host.epochs_completed,) for _ in range(7)]
    after_host = np.random.uniform()
    np.random.seed(3)
    dev = DevicePointCloudDataSet(pcs, noise=noisy, labels=labels, device=DEV)
    assert (dev.num_examples, dev.n_points, dev.epochs_completed) == (11, 64, 0)
    for k, (h_pc, h_lab, h_noisy, h_epochs) in enumerate(host_batches):
        clean, lab, feed = dev.next_batch(4)
        assert np.array_equal(_bits(clean.cpu().numpy()), _bits(h_pc)), k
        assert np.array_equal(_bits(feed.cpu().numpy()), _bits(h_noisy)), k
        assert list(lab) == list(h_lab) and dev.epochs_completed == h_epochs, k
    assert host.epochs_completed == 3
    assert np.random.uniform() == after_host                       # the same draws from numpy's global generator
    assert np.array_equal(dev.labels, host.labels)
    # a rank's slice of the global batch; without a noisy copy clean and feed are one tensor
    np.random.seed(3)
    whole = DevicePointCloudDataSet(pcs, labels=labels, device=DEV)
    np.random.seed(3)
    sliced = DevicePointCloudDataSet(pcs, labels=labels, device=DEV)
    c, l, f = whole.next_batch(4)
    assert c is f
    c1, l1, _ = sliced.next_batch(4, rank_slice=(1, 2))
    assert np.array_equal(_bits(c1.cpu().numpy()), _bits(c.cpu().numpy()[2:])) and list(l1) == list(l[2:])
    with pytest.raises(ValueError):
        DevicePointCloudDataSet(pcs, labels=labels[:3], device=DEV)


def test_device_set_augments_in_the_batch_s_launch():
    from geometric_adv_amd import ops
    from geometric_adv_amd.device_data import Augmentation, DevicePointCloudDataSet
    pcs = _clouds(10, 7, 64)
    ds = DevicePointCloudDataSet(pcs, device=DEV, init_shuffle=False)
    augment = Augmentation(gauss_mu=0.01, gauss_sigma=0.02, z_rotate=True, seed=5)
    np.random.seed(12)
    clean, _, feed = ds.next_batch(4, augment=augment, counter=9, slot_offset=4)
    after = np.random.uniform()
    np.random.seed(12)
    R = np.random.uniform(size=3)[0] * 2.0 * np.pi
    assert np.random.uniform() == after                            # three draws from the global stream, none for the noise
    R = np.array([[np.cos(R), np.sin(R), 0.0], [-np.sin(R), np.cos(R), 0.0], [0.0, 0.0, 1.0]])
    want = ops.batch_gather(_dev(pcs), [0, 1, 2, 3], dict(seed=5, counter=9, slot_offset=4, noise_mu=0.01, noise_sigma=0.02), rot=R)
    assert np.array_equal(_bits(feed.cpu().numpy()), _bits(want.cpu().numpy()))
    assert np.array_equal(_bits(clean.cpu().numpy()), _bits(pcs[:4]))


# ---- the trainer -------------------------------------------------------------------------------------------------------
def _trainer(n=64, b=4):
    from geometric_adv_amd.trainer import PointNetAETrainer, initial_weights
    return PointNetAETrainer(initial_weights(n, seed=2), n, batch_size=b, device=DEV, max_workgroups=2)


def test_trainer_on_the_device_set_equals_the_host_set():
    from geometric_adv_amd.device_data import DevicePointCloudDataSet
    from geometric_adv_amd.in_out import PointCloudDataSet
    pcs = _clouds(13, 11, 64)
    np.random.seed(3)
    a = _trainer()
    stats_a = a.train(PointCloudDataSet(pcs), 2)
    np.random.seed(3)
    b = _trainer()
    stats_b = b.train(DevicePointCloudDataSet(pcs, device=DEV), 2)
    assert [s[:2] for s in stats_a] == [s[:2] for s in stats_b]
    pa, pb = a.parameter_buffer().cpu().numpy(), b.parameter_buffer().cpu().numpy()
    assert np.array_equal(_bits(pa), _bits(pb))
    assert not np.array_equal(pa, _trainer().parameter_buffer().cpu().numpy())


def test_trainer_denoising_step_is_partial_fit_of_feed_and_clean():
    from geometric_adv_amd import ops
    from geometric_adv_amd.device_data import Augmentation, DevicePointCloudDataSet
    pcs = _clouds(14, 7, 64)
    augment = Augmentation(gauss_sigma=0.02, seed=6)
    a = _trainer()
    loss_a, _ = a._single_epoch_train(DevicePointCloudDataSet(pcs, device=DEV, init_shuffle=False), augment=augment, denoising=True)
    grads_a = a.gradients()
    clean, feed = ops.batch_gather(_dev(pcs), [0, 1, 2, 3], dict(seed=6, counter=0, noise_sigma=0.02), want_clean=True)
    assert np.array_equal(_bits(clean.cpu().numpy()), _bits(pcs[:4])) and np.mean(feed.cpu().numpy() == pcs[:4]) < 0.01
    b = _trainer()
    _, loss_b = b.partial_fit(feed, clean, want_recon=False)
    grads_b = b.gradients()
    assert loss_a == loss_b
    for group in a.GROUPS:
        for ga, gb in zip(grads_a[group], grads_b[group]):
            assert np.array_equal(_bits(ga), _bits(gb)), group
    assert np.array_equal(_bits(a.parameter_buffer().cpu().numpy()), _bits(b.parameter_buffer().cpu().numpy()))
    # the un-augmented step is another step
    c = _trainer()
    _, loss_c = c.partial_fit(pcs[:4], want_recon=False)
    assert loss_c != loss_a
    assert not np.array_equal(c.gradients()["dec_w"][2], grads_a["dec_w"][2])
    # the second epoch draws with the next counter; a host array with the same augmentation takes the same steps
    d = _trainer()
    loss_d, _ = d._single_epoch_train(pcs, augment=augment, denoising=True)
    assert loss_d == loss_a
    a._single_epoch_train(DevicePointCloudDataSet(pcs, device=DEV, init_shuffle=False), augment=augment, denoising=True)
    d._single_epoch_train(pcs, augment=augment, denoising=True)
    assert a._batches_served == d._batches_served == 2
    assert np.array_equal(_bits(a.parameter_buffer().cpu().numpy()), _bits(d.parameter_buffer().cpu().numpy()))


# ---- the command lines -------------------------------------------------------------------------------------------------
def test_train_ae_cli_with_device_data_denoising_noise_and_rotation(tmp_path):
    from geometric_adv_amd import train_ae, tf_checkpoint
    np.save(tmp_path / "clouds.npy", _clouds(15, 11, 64))
    common = ["--train_data", str(tmp_path / "clouds.npy"), "--training_epochs", "2", "--batch_size", "4"]
    stats = train_ae.main(common + ["--train_folder", str(tmp_path / "ae"), "--device_data", "1", "--denoising", "1",
                                    "--gauss_augment_sigma", "0.02", "--z_rotate", "1"])
    assert len(stats) == 2 and all(np.isfinite(s[1]) for s in stats)
    for epoch in (1, 2):
        assert os.path.exists(tmp_path / "ae" / ("models.ckpt-%d.index" % epoch))
    assert len(open(tmp_path / "ae" / "train_stats.txt").read().strip().splitlines()) == 2
    conf = json.load(open(tmp_path / "ae" / "configuration.json"))
    assert (conf["denoising"], conf["z_rotate"], conf["gauss_augment"]) == (True, True, {"mu": 0.0, "sigma": 0.02})
    w = tf_checkpoint.restore_ae_weights(str(tmp_path / "ae"), 2)
    assert all(np.isfinite(v).all() for v in w.values())
    # resident clouds alone change nothing: the run equals the host run
    plain = train_ae.main(common + ["--train_folder", str(tmp_path / "host")])
    resident = train_ae.main(common + ["--train_folder", str(tmp_path / "resident"), "--device_data", "1"])
    assert [s[:2] for s in plain] == [s[:2] for s in resident] and [s[1] for s in plain] != [s[1] for s in stats]
    assert "denoising" not in json.load(open(tmp_path / "resident" / "configuration.json"))


def test_train_classifier_cli_with_jitter_on_device(tmp_path):
    from geometric_adv_amd import train_classifier
    rng = np.random.default_rng(16)
    for split, count in (("train", 10), ("val", 4)):
        np.save(tmp_path / ("%s_x.npy" % split), (rng.random((count, 64, 3)) - 0.5).astype(np.float32))
        np.save(tmp_path / ("%s_y.npy" % split), rng.integers(0, 3, count))
    common = ["--num_point", "64", "--batch_size", "4", "--num_classes", "3", "--max_epoch", "2", "--save_model_interval", "2",
              "--train_data", "train_x.npy", "--train_labels", "train_y.npy", "--val_data", "val_x.npy", "--val_labels", "val_y.npy",
              "--top_dir", str(tmp_path), "--seed", "4"]
    logs = []
    for run in ("a", "b"):
        train_classifier.main(common + ["--jitter_on_device", "1", "--log_dir", "log_" + run])
        assert (tmp_path / ("log_" + run) / "model-002.ckpt.index").exists()
        logs.append(open(tmp_path / ("log_" + run) / "log_train.txt").read().strip().splitlines()[1:])
    losses = [float(line.split(":")[1]) for line in logs[0] if line.startswith("mean loss:")]
    assert len(losses) == 2 and np.all(np.isfinite(losses))
    assert [l for l in logs[0] if not l.startswith("Model saved")] == [l for l in logs[1] if not l.startswith("Model saved")]
    train_classifier.main(common + ["--log_dir", "log_host"])
    host = open(tmp_path / "log_host" / "log_train.txt").read().strip().splitlines()[1:]
    assert [l for l in host if l.startswith("mean loss:")] != [l for l in logs[0] if l.startswith("mean loss:")]
