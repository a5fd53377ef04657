"""The dataset stage on the host: src/in_out.py and the reader half of external/python_plyfile -- the ShapeNet
PLY folder reader, the 85/5/10 split and PointCloudDataSet.  Pure numpy; pinned to the reference by tests/golden/dataset.npz.

The PLY reader is this project's own, written from the format description (a header of `format`, `comment`, `obj_info`,
`element <name> <count>` and `property [list <count type>] <type> <name>` lines up to `end_header`, then the elements in
header order: one line of numbers per entry in an `ascii` file, packed values in header order in a binary one).  It reads
what the pipeline needs: the x, y, z of the `vertex` element.

File order is a decision of this project.  The reference takes the files in os.walk order, which is the directory order of the
file system, so its shuffled split differs from machine to machine.  Here every loader takes `file_order`: 'sorted' (the
default) sorts the files by full path and makes the split reproducible; 'walk' is the reference's behaviour.

The shuffles use numpy's global legacy generator (np.random.seed / np.random.shuffle) exactly as the reference does, so
split_data(seed=42) and PointCloudDataSet.shuffle_data(seed=55) give the reference's permutations.
"""
import os
import os.path as osp
import re
import warnings
from concurrent.futures import ThreadPoolExecutor

import numpy as np

MAX_READ_THREADS = 8        # the reference's n_threads=8 (in_out.py:116); never sized by the machine's CPU count

snc_synth_id_to_category = {
    '02691156': 'airplane',     '02773838': 'bag',        '02801938': 'basket',
    '02808440': 'bathtub',      '02818832': 'bed',        '02828884': 'bench',
    '02834778': 'bicycle',      '02843684': 'birdhouse',  '02871439': 'bookshelf',
    '02876657': 'bottle',       '02880940': 'bowl',       '02924116': 'bus',
    '02933112': 'cabinet',      '02747177': 'trash_bin',  '02942699': 'camera',
    '02954340': 'cap',          '02958343': 'car',        '03001627': 'chair',
    '03046257': 'clock',        '03207941': 'dishwasher', '03211117': 'display',
    '04379243': 'table',        '04401088': 'telephone',  '02946921': 'can',
    '04460130': 'tower',        '04468005': 'train',      '03085013': 'keyboard',
    '03261776': 'earphone',     '03325088': 'faucet',     '03337140': 'file_cabinet',
    '03467517': 'guitar',       '03513137': 'helmet',     '03593526': 'jar',
    '03624134': 'knife',        '03636649': 'lamp',       '03642806': 'laptop',
    '03691459': 'loudspeaker',  '03710193': 'mailbox',    '03759954': 'microphone',
    '03761084': 'microwaves',   '03790512': 'motorbike',  '03797390': 'mug',
    '03928116': 'piano',        '03938244': 'pillow',     '03948459': 'pistol',
    '03991062': 'flowerpot',    '04004475': 'printer',    '04074963': 'remote',
    '04090263': 'rifle',        '04099429': 'rocket',     '04225987': 'skateboard',
    '04256520': 'sofa',         '04330267': 'stove',      '04530566': 'watercraft',
    '04554684': 'washer',       '02858304': 'boat',       '02992529': 'cellphone'
}


def snc_category_to_synth_id():
    return {v: k for k, v in snc_synth_id_to_category.items()}


def create_dir(dir_path):
    os.makedirs(dir_path, exist_ok=True)
    return dir_path


# ---------------------------------------------------------------------------------------------------------------------
# PLY
# ---------------------------------------------------------------------------------------------------------------------
_PLY_TYPES = {'char': 'i1', 'int8': 'i1', 'uchar': 'u1', 'uint8': 'u1', 'short': 'i2', 'int16': 'i2', 'ushort': 'u2',
              'uint16': 'u2', 'int': 'i4', 'int32': 'i4', 'uint': 'u4', 'uint32': 'u4', 'float': 'f4', 'float32': 'f4',
              'double': 'f8', 'float64': 'f8'}
_PLY_FORMATS = {'ascii': None, 'binary_little_endian': '<', 'binary_big_endian': '>'}


def _parse_ply_header(data, file_name):
    """-> (format key, [(element name, count, [(property name, numpy type code or None for a list)])], body offset)."""
    if data[:3] != b'ply' or data[3:4] not in (b'\n', b'\r'):
        raise ValueError("%s: not a PLY file (no 'ply' magic line)" % file_name)
    fmt, elements, pos = None, [], 0
    while True:
        end = data.find(b'\n', pos)
        if end < 0:
            raise ValueError("%s: truncated header (no end_header line)" % file_name)
        line = data[pos:end].decode('ascii', 'replace').strip()
        pos = end + 1
        tok = line.split()
        if not tok or tok[0] in ('ply', 'comment', 'obj_info'):
            continue
        if tok[0] == 'end_header':
            break
        if tok[0] == 'format':
            if len(tok) != 3 or tok[1] not in _PLY_FORMATS or tok[2] != '1.0':
                raise ValueError("%s: unknown format line %r" % (file_name, line))
            fmt = tok[1]
        elif tok[0] == 'element':
            if len(tok) != 3 or not tok[2].isdigit():
                raise ValueError("%s: malformed element line %r" % (file_name, line))
            elements.append((tok[1], int(tok[2]), []))
        elif tok[0] == 'property':
            if not elements:
                raise ValueError("%s: property line %r before any element" % (file_name, line))
            if len(tok) == 5 and tok[1] == 'list' and tok[2] in _PLY_TYPES and tok[3] in _PLY_TYPES:
                elements[-1][2].append((tok[4], None))
            elif len(tok) == 3 and tok[1] in _PLY_TYPES:
                elements[-1][2].append((tok[2], _PLY_TYPES[tok[1]]))
            else:
                raise ValueError("%s: malformed property line %r" % (file_name, line))
        else:
            raise ValueError("%s: unknown header line %r" % (file_name, line))
    if fmt is None:
        raise ValueError("%s: unknown format (the header has no format line)" % file_name)
    return fmt, elements, pos


def load_ply(file_name):
    """in_out.py:79-82: the points of a PLY file, float32 (n, 3) = np.vstack([x, y, z]).T of its `vertex` element.
    Reads ascii, binary_little_endian and binary_big_endian files; x, y, z may be float or double and sit anywhere among the
    vertex properties; other scalar vertex properties are skipped and the elements after `vertex` are not read.  Raises
    ValueError with the reason for anything else."""
    with open(file_name, 'rb') as f:
        data = f.read()
    fmt, elements, pos = _parse_ply_header(data, file_name)
    names = [e[0] for e in elements]
    if 'vertex' not in names:
        raise ValueError("%s: no vertex element" % file_name)
    vi = names.index('vertex')
    _, count, props = elements[vi]
    if any(code is None for _, code in props):
        raise ValueError("%s: a list property inside the vertex element is not supported" % file_name)
    pnames = [p for p, _ in props]
    for axis in 'xyz':
        if axis not in pnames:
            raise ValueError("%s: the vertex element has no %r property" % (file_name, axis))
        if dict(props)[axis] not in ('f4', 'f8'):
            raise ValueError("%s: vertex property %r must be float or double" % (file_name, axis))
    if fmt == 'ascii':
        lines = data[pos:].split(b'\n')
        skip = sum(e[1] for e in elements[:vi])
        rows = lines[skip:skip + count]
        if len(rows) < count or (count and not rows[-1].strip()):
            raise ValueError("%s: truncated body (%d vertex lines expected)" % (file_name, count))
        cols = [pnames.index(a) for a in 'xyz']
        out = np.empty((count, 3), np.float32)
        for k, row in enumerate(rows):
            fields = row.split()
            if len(fields) < len(props):
                raise ValueError("%s: truncated body (vertex %d has %d of %d values)" % (file_name, k, len(fields), len(props)))
            for j, c in enumerate(cols):
                out[k, j] = np.dtype(props[c][1]).type(float(fields[c]))
        return out
    order = _PLY_FORMATS[fmt]
    for name, n, eprops in elements[:vi]:
        if any(code is None for _, code in eprops):
            raise ValueError("%s: element %r with a list property comes before vertex in a binary file: its size is not "
                             "known without reading it" % (file_name, name))
        pos += n * sum(np.dtype(code).itemsize for _, code in eprops)
    dtype = np.dtype([(p, order + code) for p, code in props])
    if pos + count * dtype.itemsize > len(data):
        raise ValueError("%s: truncated body (%d bytes of vertex data expected, %d present)"
                         % (file_name, count * dtype.itemsize, max(len(data) - pos, 0)))
    v = np.frombuffer(data, dtype=dtype, count=count, offset=pos)
    return np.vstack([v['x'], v['y'], v['z']]).T.astype(np.float32)


# ---------------------------------------------------------------------------------------------------------------------
# folders, the split and the data set.  Signatures, return values and random streams are the reference's (src/in_out.py);
# pinned by tests/golden/dataset.npz.
# ---------------------------------------------------------------------------------------------------------------------
SPLIT_FRACTIONS = (.85, .05, .10)
FILE_ORDERS = ('sorted', 'walk')


def _legacy_permutation(count, seed=None):
    """A permutation of range(count) from numpy's GLOBAL legacy generator, reseeded first if a seed is given: the stream every
    shuffle of the reference's dataset stage draws from, which is what makes seed 42 / seed 55 reproduce its orders."""
    if seed is not None:
        np.random.seed(seed)
    order = np.arange(count)
    np.random.shuffle(order)
    return order


def files_in_subdirs(top_dir, search_pattern, file_order='sorted'):
    """Iterator over the full names, under top_dir at any depth, that the regular expression matches.  file_order 'sorted'
    (default): by full path; 'walk': as os.walk meets them (the reference's order, which depends on the file system)."""
    if file_order not in FILE_ORDERS:
        raise ValueError("file_order must be one of %s, not %r" % (FILE_ORDERS, file_order))
    wanted = re.compile(search_pattern)
    met = (osp.join(folder, name) for folder, _, names in os.walk(top_dir) for name in names)
    hits = (full for full in met if wanted.search(full))
    return iter(sorted(hits)) if file_order == 'sorted' else hits


def pc_loader(f_name):
    """One file of ShapeNet's layout <synset id>/<model id>.ply -> (points (n, 3), model id, synset id)."""
    folder, base = osp.split(f_name)
    return load_ply(f_name), base.partition('.')[0], osp.basename(folder)


def load_point_clouds_from_filenames(file_names, n_threads, loader, verbose=False):
    """-> (clouds float32 (k, n, 3), model ids, synset ids; the last two object arrays) in the order of file_names.  Every
    file must hold as many points as the first.  Read by min(n_threads, 8) threads."""
    file_names = list(file_names)
    workers = max(1, min(int(n_threads), MAX_READ_THREADS))
    with ThreadPoolExecutor(workers) as pool:
        loaded = list(pool.map(loader, file_names))
    shape = loaded[0][0].shape
    for name, item in zip(file_names, loaded):
        if item[0].shape != shape:
            raise ValueError("%s holds a cloud of shape %s, the first file one of %s" % (name, item[0].shape, shape))
    clouds = np.stack([item[0] for item in loaded]).astype(np.float32, copy=False)
    models = np.array([item[1] for item in loaded] + [None], dtype=object)[:-1]
    synsets = np.array([item[2] for item in loaded] + [None], dtype=object)[:-1]
    if len(set(models)) < len(models):
        warnings.warn("%d of the %d model ids occur more than once" % (len(models) - len(set(models)), len(models)))
    if verbose:
        print("read %d clouds of %d shape classes" % (len(clouds), len(set(synsets))))
    return clouds, models, synsets


def split_data(data, split, seed, perm=None):
    """-> (train, val, test, perm).  data[perm] is cut at int(split[0] * n + 0.5) and int((split[0] + split[1]) * n + 0.5).
    perm: the permutation to use (then the seed is ignored); None draws it from the legacy generator seeded with `seed`."""
    n = len(data)
    if sum(split) != 1.:
        raise ValueError("the split fractions %s add up to %r, not 1" % (tuple(split), sum(split)))
    if perm is None:
        perm = _legacy_permutation(n, seed)
    elif len(perm) != n:
        raise ValueError("a permutation of %d entries cannot order %d examples" % (len(perm), n))
    first_cut = int(split[0] * n + 0.5)
    second_cut = int((split[0] + split[1]) * n + 0.5)
    ordered = data[perm]
    return ordered[:first_cut], ordered[first_cut:second_cut], ordered[second_cut:], perm


def _read_class_folder(top_dir, n_threads, file_ending, verbose, file_order):
    names = list(files_in_subdirs(top_dir, file_ending, file_order))
    if not names:
        raise FileNotFoundError("no file matching %r under %s" % (file_ending, top_dir))
    return load_point_clouds_from_filenames(names, n_threads, loader=pc_loader, verbose=verbose)


def load_all_point_clouds_under_folder(top_dir, n_threads=20, file_ending='.ply', verbose=False, file_order='sorted'):
    """Every cloud under top_dir as one unshuffled data set labelled '<synset id>_<model id>'.  file_order: 'sorted' (by full
    path, the default) or 'walk' (the reference's os.walk order)."""
    clouds, models, synsets = _read_class_folder(top_dir, n_threads, file_ending, verbose, file_order)
    return PointCloudDataSet(clouds, labels=synsets + '_' + models, init_shuffle=False)


def load_and_split_all_point_clouds_under_folder(top_dir, n_threads=20, file_ending='.ply', split=SPLIT_FRACTIONS, seed=42,
                                                 verbose=False, file_order='sorted'):
    """-> (train, val, test) unshuffled data sets of the clouds under top_dir; ONE permutation orders the clouds, the model ids
    and the synset ids.  file_order: 'sorted' (by full path, the default: the same split on every machine) or 'walk' (the
    reference's os.walk order, which follows the file system)."""
    clouds, models, synsets = _read_class_folder(top_dir, n_threads, file_ending, verbose, file_order)
    *cloud_parts, perm = split_data(clouds, split, seed)
    label_parts = split_data(synsets + '_' + models, split, seed, perm)[:3]
    return tuple(PointCloudDataSet(c, labels=l, init_shuffle=False) for c, l in zip(cloud_parts, label_parts))


def load_dataset(class_names, set_type, input_dir, file_order='sorted'):
    """-> (data set, slice_idx, pc_label): the chosen split of every class, class after class in the order of class_names;
    slice_idx[i] is where class i starts (and slice_idx[-1] the total), pc_label the class index of every cloud.
    set_type: 'train_set', 'val_set', anything else = the test set.  file_order: see the module docstring."""
    which = {'train_set': 0, 'val_set': 1}.get(set_type, 2)
    synset_of = snc_category_to_synth_id()
    merged, slice_idx, pc_label = None, [0], []
    for class_index, name in enumerate(class_names):
        print('reading class %s (%s)' % (name, synset_of[name]))
        part = load_and_split_all_point_clouds_under_folder(osp.join(input_dir, synset_of[name]), n_threads=MAX_READ_THREADS,
                                                            file_ending='.ply', verbose=True, file_order=file_order)[which]
        pc_label.extend([class_index] * part.num_examples)
        slice_idx.append(len(pc_label))
        merged = part if merged is None else merged.merge(part)
    return merged, slice_idx, pc_label


class PointCloudDataSet(object):
    """Clouds (k, n, 3) with one label each and, optionally, a noisy copy of the clouds, served in batches.  Interface, default
    labels (int8 ones) and random stream are the reference's PointCloudDataSet; every shuffle draws from numpy's global legacy
    generator (_legacy_permutation)."""

    def __init__(self, point_clouds, noise=None, labels=None, copy=True, init_shuffle=True):
        if labels is not None and len(labels) != len(point_clouds):
            raise ValueError("%d labels for %d clouds" % (len(labels), len(point_clouds)))
        if noise is not None and not isinstance(noise, np.ndarray):
            raise TypeError("noise must be a numpy array")
        own = (lambda a: a.copy()) if copy else (lambda a: a)
        self.point_clouds = own(point_clouds)
        self.labels = np.ones(len(point_clouds), dtype=np.int8) if labels is None else own(labels)
        self.noisy_point_clouds = None if noise is None else own(noise)
        self.num_examples, self.n_points = point_clouds.shape[0], point_clouds.shape[1]
        self.epochs_completed = 0
        self._cursor = 0                      # where the next batch starts
        if init_shuffle:
            self.shuffle_data()

    def _reorder(self, order):
        self.point_clouds = self.point_clouds[order]
        self.labels = self.labels[order]
        if self.noisy_point_clouds is not None:
            self.noisy_point_clouds = self.noisy_point_clouds[order]

    def shuffle_data(self, seed=None):
        """Reorders the examples (clouds, labels and noisy clouds alike); returns self."""
        self._reorder(_legacy_permutation(self.num_examples, seed))
        return self

    def shuffle_points(self, seed=None):
        """Reorders the points inside every cloud, in place.  ONE index array is shuffled again for each cloud, so cloud i's
        order is the composition of the first i + 1 shuffles (the reference's stream); returns self."""
        if seed is not None:
            np.random.seed(seed)
        order = np.arange(self.n_points)
        for k in range(self.num_examples):
            np.random.shuffle(order)
            self.point_clouds[k] = self.point_clouds[k][order]
            if self.noisy_point_clouds is not None:
                self.noisy_point_clouds[k] = self.noisy_point_clouds[k][order]
        return self

    def next_batch(self, batch_size, shuffle=True, seed=None):
        """-> (clouds, labels, noisy clouds or None) of the next batch_size examples.  A batch that would run past the end is
        not cut short: the epoch counts as completed, the set is reshuffled (if `shuffle`) and the batch is its first
        batch_size examples."""
        if self._cursor + batch_size > self.num_examples:
            self.epochs_completed += 1
            if shuffle:
                self.shuffle_data(seed)
            self._cursor = 0
        window = slice(self._cursor, self._cursor + batch_size)
        self._cursor += batch_size
        noisy = None if self.noisy_point_clouds is None else self.noisy_point_clouds[window]
        return self.point_clouds[window], self.labels[window], noisy

    def full_epoch_data(self, shuffle=True, seed=None):
        """-> copies (clouds, labels, noisy clouds or None) of the whole set, in a fresh random order if `shuffle`; the set
        itself keeps its order."""
        order = _legacy_permutation(self.num_examples, seed) if shuffle else np.arange(self.num_examples)
        noisy = None if self.noisy_point_clouds is None else self.noisy_point_clouds[order]
        return self.point_clouds[order], self.labels[order], noisy

    def merge(self, other_data_set):
        """Appends another set's examples and starts the epoch bookkeeping afresh; returns self.  The labels stay
        one-dimensional for every size (the reference squeezes them, which leaves a 0-d array when the merged set holds ONE
        example, and its own shuffle_data then fails)."""
        other = other_data_set
        self.point_clouds = np.concatenate([self.point_clouds, other.point_clouds], axis=0)
        self.labels = np.concatenate([np.reshape(self.labels, -1), np.reshape(other.labels, -1)])
        if self.noisy_point_clouds is not None:
            self.noisy_point_clouds = np.concatenate([self.noisy_point_clouds, other.noisy_point_clouds], axis=0)
        self.num_examples = len(self.point_clouds)
        self._cursor, self.epochs_completed = 0, 0
        return self
