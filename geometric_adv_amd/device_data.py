"""Device-resident training batches: the data side of victim-AE training (src/in_out.py PointCloudDataSet, src/general_utils.py
apply_augmentations / rand_rotation_matrix, src/pointnet_ae.py:114-128) with the clouds kept on the GPU.

The clouds are uploaded once.  A shuffle reorders a host index array, never the clouds; a batch is ONE launch of
ops.batch_gather (csrc/dataset.hip): gather by index, Gaussian noise, rotation.

Random streams.  Shuffles draw from numpy's global legacy generator exactly as in_out.PointCloudDataSet does, and with z_rotate
one matrix per batch comes from rand_rotation_matrix(): three uniforms of the same stream, as in the reference.  A run with
z_rotate alone therefore keeps the reference's shuffle orders.  The Gaussian noise is the device generator's (csrc/dataset.hip:
same distribution as np.random.normal, not the same draws, keyed by Augmentation.seed, the caller's batch counter and the
output slot).  The reference's np.random.normal(mu, sigma, batch.shape) draws are not made, so a run WITH noise leaves numpy's
stream -- and with it every later shuffle and rotation -- different from the reference's.
"""
import numpy as np
import torch

from . import ops
from .in_out import _legacy_permutation


class Augmentation(object):
    """Configuration.gauss_augment ({'mu', 'sigma'}) and Configuration.z_rotate of the reference, and the noise generator's seed.
    clip: None = the reference's unclamped noise; a positive value clamps sigma * g to [-clip, clip] (the classifier's jitter)."""

    def __init__(self, gauss_mu=0.0, gauss_sigma=0.0, clip=None, z_rotate=False, seed=0):
        if not gauss_sigma >= 0:
            raise ValueError("gauss_sigma must be >= 0, got %r" % (gauss_sigma,))
        if clip is not None and not clip > 0:
            raise ValueError("clip must be positive or None, got %r" % (clip,))
        self.gauss_mu, self.gauss_sigma, self.clip = float(gauss_mu), float(gauss_sigma), clip
        self.z_rotate, self.seed = bool(z_rotate), int(seed)

    @property
    def active(self):
        return self.gauss_sigma > 0 or self.z_rotate

    def fields(self, counter=0, slot_offset=0, rotate_first=False):
        """The fields of ops.BatchAugment for one batch."""
        return dict(seed=self.seed % (1 << 64), counter=int(counter) % (1 << 64), slot_offset=int(slot_offset),
                    noise_mu=self.gauss_mu, noise_sigma=self.gauss_sigma, noise_clip=float(self.clip or 0.0),
                    rotate_first=int(bool(rotate_first)))

    def draw_rotation(self):
        """The batch's matrix (three draws from numpy's global stream), or None without z_rotate."""
        return rand_rotation_matrix() if self.z_rotate else None


def rand_rotation_matrix(deflection=1.0, z_only=True, seed=None):
    """A random rotation matrix from three uniforms (u0, u1, u2) of numpy's global generator (reseeded first if a seed is
    given), after Arvo's "Fast random rotation matrices" (Graphics Gems III): R turns by theta = 2 pi deflection u0 about z,
    [[c, s, 0], [-s, c, 0], [0, 0, 1]].  z_only returns R.  Otherwise the pole is deflected: with phi = 2 pi u1, w = 2 deflection u2
    and v = (sin(phi) sqrt(w), cos(phi) sqrt(w), sqrt(2 - w)) the result is (v v^T - I) R."""
    if seed is not None:
        np.random.seed(seed)
    u0, u1, u2 = np.random.uniform(size=(3,))
    theta = u0 * 2.0 * deflection * np.pi
    c, s = np.cos(theta), np.sin(theta)
    about_z = np.array([[c, s, 0.0], [-s, c, 0.0], [0.0, 0.0, 1.0]])
    if z_only:
        return about_z
    phi, w = u1 * 2.0 * np.pi, u2 * 2.0 * deflection
    v = np.array([np.sin(phi) * np.sqrt(w), np.cos(phi) * np.sqrt(w), np.sqrt(2.0 - w)])
    return (np.outer(v, v) - np.eye(3)).dot(about_z)


def gather_augmented(data, index, augment, counter=0, slot_offset=0, want_clean=False, clean_data=None):
    """ops.batch_gather of the GPU clouds `data` under an Augmentation (None = plain gather), in the auto-encoder's order: noise,
    then the batch's rotation.  clean_data: where `clean` comes from when it is not `data` (the set has a noisy copy)."""
    aug = rot = None
    if augment is not None and augment.active:
        aug = augment.fields(counter, slot_offset)
        rot = augment.draw_rotation()
    if clean_data is not None and want_clean:
        return ops.batch_gather(clean_data, index), ops.batch_gather(data, index, aug, rot)
    return ops.batch_gather(data, index, aug, rot, want_clean=want_clean)


class DevicePointCloudDataSet(object):
    """in_out.PointCloudDataSet with the clouds (and the optional noisy copy) resident on the GPU: the same bookkeeping and the
    same draws from numpy's global generator, so under one seed it serves the host set's batches bit for bit.  The clouds never
    move; `order` (host) maps position to cloud and a shuffle composes a permutation into it.  Labels stay on the host."""

    device_resident = True

    def __init__(self, point_clouds, noise=None, labels=None, device=None, init_shuffle=True):
        if labels is not None and len(labels) != len(point_clouds):
            raise ValueError("%d labels for %d clouds" % (len(labels), len(point_clouds)))
        self.device = torch.device(device if device is not None else "cuda:0")
        self.point_clouds = self._upload(point_clouds)
        if self.point_clouds.dim() != 3 or self.point_clouds.shape[2] != 3:
            raise ValueError("point_clouds must be (k, n, 3); got %s" % (tuple(self.point_clouds.shape),))
        self.noisy_point_clouds = None if noise is None else self._upload(noise)
        if self.noisy_point_clouds is not None and self.noisy_point_clouds.shape != self.point_clouds.shape:
            raise ValueError("the noisy copy must have the clouds' shape")
        self.all_labels = np.ones(len(point_clouds), dtype=np.int8) if labels is None else np.array(labels)
        self.num_examples, self.n_points = int(self.point_clouds.shape[0]), int(self.point_clouds.shape[1])
        self.order = np.arange(self.num_examples)
        self.epochs_completed = 0
        self._cursor = 0
        if init_shuffle:
            self.shuffle_data()

    def _upload(self, a):
        if isinstance(a, torch.Tensor):
            return a.to(self.device, dtype=torch.float32).contiguous()
        return torch.from_numpy(np.ascontiguousarray(a, dtype=np.float32)).to(self.device)

    @property
    def labels(self):
        """The labels in the set's current order (host)."""
        return self.all_labels[self.order]

    def shuffle_data(self, seed=None):
        """Reorders the examples: a permutation from numpy's global generator composed into `order`; returns self."""
        self.order = self.order[_legacy_permutation(self.num_examples, seed)]
        return self

    def set_order(self, order):
        """Serves the resident clouds `order` (any index array into them) from the start: num_examples becomes len(order)."""
        order = np.asarray(order)
        if order.ndim != 1 or order.dtype.kind not in "iu" or (order.size and (order.min() < 0 or order.max() >= len(self.all_labels))):
            raise ValueError("order must be a one-dimensional array of indices below %d" % len(self.all_labels))
        self.order, self.num_examples, self._cursor = order, int(order.size), 0
        return self

    def next_batch(self, batch_size, shuffle=True, seed=None, augment=None, counter=0, slot_offset=0, rank_slice=None,
                   from_noisy=True):
        """-> (clean, labels, feed) of the next batch_size examples, wrapping and reshuffling as PointCloudDataSet.next_batch.
        clean and feed are GPU tensors (the same tensor where nothing distinguishes them), labels a host array.  feed is
        gathered from the noisy copy when there is one (and from_noisy) and augmented by `augment` (an Augmentation) with the
        generator keyed by (augment.seed, counter, slot_offset + position in the batch).  rank_slice = (rank, world): the batch
        is the global one and only positions rank * batch_size / world ... of it are gathered; the caller passes that start
        as slot_offset so that the ranks together draw one rank's noise for the whole batch."""
        if self._cursor + batch_size > self.num_examples:
            self.epochs_completed += 1
            if shuffle:
                self.shuffle_data(seed)
            self._cursor = 0
        index = self.order[self._cursor:self._cursor + batch_size]
        self._cursor += batch_size
        if rank_slice is not None:
            rank, world = rank_slice
            if batch_size % world:
                raise ValueError("a batch of %d does not divide over %d ranks" % (batch_size, world))
            local = batch_size // world
            index = index[rank * local:(rank + 1) * local]
        noisy = self.noisy_point_clouds if from_noisy else None
        active = augment is not None and augment.active
        if noisy is None and not active:
            feed = ops.batch_gather(self.point_clouds, index)
            return feed, self.all_labels[index], feed
        if noisy is None:
            clean, feed = gather_augmented(self.point_clouds, index, augment, counter, slot_offset, want_clean=True)
        else:
            clean, feed = gather_augmented(noisy, index, augment, counter, slot_offset, want_clean=True, clean_data=self.point_clouds)
        return clean, self.all_labels[index], feed


class CloudAugmenter(object):
    """The reference's AtlasNet Augmenter (transfer/atlasnet/dataset/augmenter.py) with its argument names, on resident clouds:
    one ops.augment_batch launch per batch.  rotation_axis and flips are sequences of axes out of 0, 1, 2 (the axial rotations
    are applied in ascending axis order); the operators come in the Augmenter's order and with its ranges.  The draws are the
    device generator's (csrc/dataset.hip), keyed by (seed, the caller's batch counter, output slot): the reference's
    distributions, not torch's numbers."""

    def __init__(self, translation=False, rotation_axis=(), rotation_3D=False, anisotropic_scaling=False, flips=(), seed=0):
        self.rotation_axis, self.flips = self._axes(rotation_axis, "rotation_axis"), self._axes(flips, "flips")
        for name, v in (("translation", translation), ("rotation_3D", rotation_3D), ("anisotropic_scaling", anisotropic_scaling)):
            if not isinstance(v, (bool, np.bool_)):
                raise ValueError("%s must be True or False, got %r" % (name, v))
        self.translation, self.rotation_3D, self.anisotropic_scaling = bool(translation), bool(rotation_3D), bool(anisotropic_scaling)
        self.seed = int(seed)

    @staticmethod
    def _axes(axes, name):
        axes = list(axes)
        if any(isinstance(a, bool) or not isinstance(a, (int, np.integer)) or not 0 <= a <= 2 for a in axes) or len(set(axes)) != len(axes):
            raise ValueError("%s must hold distinct axes out of 0, 1, 2; got %r" % (name, axes))
        return tuple(sorted(int(a) for a in axes))

    @property
    def active(self):
        return bool(self.translation or self.rotation_axis or self.rotation_3D or self.anisotropic_scaling or self.flips)

    def fields(self, counter=0, slot_offset=0):
        """The fields of ops.CloudAugment for one batch (sample is left to ops.augment_batch)."""
        return dict(seed=self.seed % (1 << 64), counter=int(counter) % (1 << 64), slot_offset=int(slot_offset),
                    rot_axes=sum(1 << a for a in self.rotation_axis), rot_3d=int(self.rotation_3D), scale=int(self.anisotropic_scaling),
                    flip_axes=sum(1 << a for a in self.flips), translate=int(self.translation))

    def __call__(self, data, index, counter, slot_offset=0, sample_points=None):
        """-> the batch (len(index), sample_points or data's points, 3) on the GPU: data[index], re-sampled with replacement
        when sample_points is given, under this augmenter's operators."""
        fields = self.fields(counter, slot_offset)
        if sample_points:
            fields["sample"] = 1
        return ops.augment_batch(data, index, fields, n_out=sample_points or None)
