"""CPU: the host side of the device-resident training batches -- the statistics of the noise generator's definition
(tests/_batch_noise64.py, the float64 restatement of csrc/dataset.hip's header), that its values belong to the slot and not to
the batch, rand_rotation_matrix, and the new flags of train_ae and train_classifier."""
import math

import numpy as np
import pytest

import _batch_noise64 as BN

SLOTS, POINTS = 8, 2731            # 8 x 2731 x 3 = 65 544 draws


@pytest.mark.parametrize("seed,counter", [(7, 0), (7, 1)])
def test_generator_statistics(seed, counter):
    g = BN.normals(seed, counter, np.arange(SLOTS), POINTS)
    flat = g.reshape(-1)
    n = flat.size
    assert n == 65544 and np.all(np.isfinite(flat))
    mean, var = flat.mean(), flat.var()
    print("mean %.3e (limit %.3e), var - 1 %.3e (limit %.3e)" % (mean, 4 / math.sqrt(n), var - 1, 4 * math.sqrt(2 / n)))
    assert abs(mean) < 4 / math.sqrt(n)
    assert abs(var - 1) < 4 * math.sqrt(2 / n)
    srt = np.sort(flat)
    cdf = 0.5 * (1.0 + np.frompyfunc(math.erf, 1, 1)(srt / math.sqrt(2.0)).astype(np.float64))
    ks = max(np.max(np.arange(1, n + 1) / n - cdf), np.max(cdf - np.arange(0, n) / n))
    print("KS %.3e (limit %.3e)" % (ks, 1.63 / math.sqrt(n)))
    assert ks < 1.63 / math.sqrt(n)
    corr = np.corrcoef(g.reshape(-1, 3).T)
    worst = np.abs(corr - np.eye(3)).max()
    print("largest correlation between coordinates %.3e (limit %.3e)" % (worst, 4 / math.sqrt(n / 3)))
    assert worst < 4 / math.sqrt(n / 3)


def test_noise_belongs_to_the_slot_not_to_the_batch():
    five, two = BN.normals(7, 0, np.arange(5), 100), BN.normals(7, 0, np.arange(2), 100)
    assert np.array_equal(five[:2].view(np.uint64), two.view(np.uint64))
    assert np.array_equal(BN.normals(7, 0, np.array([2, 3, 4]), 100).view(np.uint64), five[2:].view(np.uint64))
    other = BN.normals(7, 1, np.arange(5), 100)
    assert not np.any(other == five)
    assert not np.any(BN.normals(8, 0, np.arange(5), 100) == five)


@pytest.mark.parametrize("seed", [0, 5, 11])
def test_rand_rotation_matrix(seed):
    from geometric_adv_amd.device_data import rand_rotation_matrix
    np.random.seed(seed)
    u = np.random.uniform(size=(3,))
    after = np.random.uniform()
    np.random.seed(seed)
    R = rand_rotation_matrix()
    assert np.random.uniform() == after, "rand_rotation_matrix must consume exactly three uniforms"
    theta = 2.0 * np.pi * u[0]
    c, s = np.cos(theta), np.sin(theta)
    assert R.dtype == np.float64 and np.array_equal(R, np.array([[c, s, 0.0], [-s, c, 0.0], [0.0, 0.0, 1.0]]))
    assert np.abs(R @ R.T - np.eye(3)).max() <= 1e-15 and abs(np.linalg.det(R) - 1.0) <= 1e-15
    assert np.array_equal(rand_rotation_matrix(seed=seed), R)               # seed= reseeds the global generator first
    np.random.seed(seed)
    M = rand_rotation_matrix(z_only=False)
    assert np.random.uniform() == after
    assert np.abs(M @ M.T - np.eye(3)).max() <= 1e-15 and not np.array_equal(M, R)
    np.random.seed(seed)
    assert np.array_equal(rand_rotation_matrix(deflection=0.0), np.eye(3))


DEFAULT_KEYS = {"n_input", "loss", "batch_size", "learning_rate", "training_epochs", "saver_step", "bneck_size", "object_class",
                "class_names", "sort_axes", "experiment_name", "held_out_step", "data_source"}


def test_train_ae_flags_and_configuration():
    from geometric_adv_amd import train_ae
    f = train_ae.parse_flags(["--train_data", "x.npy"])
    assert (f.device_data, f.denoising, f.z_rotate, f.gauss_augment_mu, f.gauss_augment_sigma) == (0, 0, 0, 0.0, 0.0)
    base = ["--data_dir", "somewhere", "--class_names", "chair", "lamp", "--sort_axes", "0", "--training_epochs", "7", "--batch_size", "4",
            "--held_out_step", "2"]
    default = {"n_input": [64, 3], "loss": "chamfer", "batch_size": 4, "learning_rate": 0.0005, "training_epochs": 7,
               "saver_step": 50, "bneck_size": 128, "object_class": ["2l"], "class_names": ["chair", "lamp"], "sort_axes": 0,
               "experiment_name": "autoencoder", "held_out_step": 2, "data_source": "data_dir"}
    assert train_ae.make_configuration(train_ae.parse_flags(base), 64) == default
    assert train_ae.make_configuration(train_ae.parse_flags(base + ["--device_data", "1"]), 64) == default
    conf = train_ae.make_configuration(train_ae.parse_flags(base + ["--z_rotate", "1"]), 64)
    assert set(conf) == DEFAULT_KEYS | {"denoising", "z_rotate", "gauss_augment"}
    assert (conf["denoising"], conf["z_rotate"], conf["gauss_augment"]) == (False, True, None)
    assert {k: conf[k] for k in DEFAULT_KEYS} == default
    conf = train_ae.make_configuration(train_ae.parse_flags(base + ["--denoising", "1", "--gauss_augment_sigma", "0.02",
                                                                    "--gauss_augment_mu", "0.1"]), 64)
    assert (conf["denoising"], conf["z_rotate"], conf["gauss_augment"]) == (True, False, {"mu": 0.1, "sigma": 0.02})
    with pytest.raises(SystemExit):
        train_ae.parse_flags(base + ["--gauss_augment_sigma", "-1"])


def test_train_classifier_accepts_jitter_on_device():
    from geometric_adv_amd import train_classifier
    p = train_classifier.build_parser()
    assert p.parse_args([]).jitter_on_device == 0
    assert p.parse_args(["--jitter_on_device", "1"]).jitter_on_device == 1


def test_augmentation_fields():
    from geometric_adv_amd.device_data import Augmentation
    a = Augmentation(gauss_mu=0.1, gauss_sigma=0.02, seed=9)
    assert a.active and not Augmentation().active and Augmentation(z_rotate=True).active
    assert a.fields(counter=4, slot_offset=8) == dict(seed=9, counter=4, slot_offset=8, noise_mu=0.1, noise_sigma=0.02,
                                                       noise_clip=0.0, rotate_first=0)
    assert a.draw_rotation() is None
    with pytest.raises(ValueError):
        Augmentation(gauss_sigma=-1.0)
    with pytest.raises(ValueError):
        Augmentation(clip=0.0)
