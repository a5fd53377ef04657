"""Writes tests/golden/dataset/ (a two-class ShapeNet-style tree of small PLY files) and tests/golden/dataset.npz from the
REFERENCE's own src/in_out.py and src/shift_rotate_util.py (TEST INFRASTRUCTURE; needs a checkout of the reference project, run
on a host that has one -- never on the GPU machines, where the tests only read the fixtures):

    python tools/make_golden_dataset.py --reference <checkout of the reference project>

The reference's modules are imported as they are (numpy and six are all they need here); `tensorflow`, which
shift_rotate_util imports for functions this tool does not call, is replaced by an empty stub.

The tree: 04379243 (table, 7 files) and 02958343 (car, 13 files), 64 points each, written by tests/_ply_writer.py in the
three formats in turn; one file with double coordinates, one with colour properties between x and y, one with normals before
x, one with a face element after vertex, some with comment / obj_info lines.

All 20 hold 64 points because the reference's folder loader needs one point count; tests/golden/dataset_sizes/ holds three
more files of 32, 47 and 63 points (one per format) for the reader alone.

dataset.npz:
  ply__<synset>__<model>            the reference's load_ply of every file (float64 for the double file)
  sizes__<name>                     the same for the three files of dataset_sizes/
  split<n>_{train,val,test,perm}    split_data(arange(n) * 3 + 1, (.85, .05, .10), 42) for n = 7, 13, 20, 4379
  <set>_{pc,labels,slice_idx,pc_label,sorted}   load_dataset(['table', 'car'], <set>, tree) with the reference's
                                    files_in_subdirs replaced by one that sorts by full path (the file order is the one thing
                                    this project decides differently), and sort_axes of those clouds (empty if the set is empty)
  sa_in, sa_out_neg{0,1}, sa_idx, sa_ref_accepts   sort_axes of 64 clouds with both neg_rot values and get_sort_axes_idx's
                                    indices.  The reference stops at its own assertion for a cloud whose x or y extent is exactly
                                    0 (its argsort then moves z): sa_ref_accepts is False there and the expected output is the
                                    project's documented rule (z stays, swapped iff ex <= ey, negated iff ex < ey), restated below.
  shuffle55_<n>                     the order PointCloudDataSet.shuffle_data(55) gives n = 1, 2, 7, 17 examples
  next_batch_ids                    ids of four next_batch(3) calls on 7 examples after shuffle_data(55): the third wraps
                                    around and reshuffles
"""
import argparse
import os
import os.path as osp
import shutil
import sys
import types

import numpy as np

ROOT = osp.dirname(osp.dirname(osp.abspath(__file__)))
sys.path.insert(0, osp.join(ROOT, 'tests'))
from _ply_writer import vertex, write_ply  # noqa: E402

TREE = osp.join(ROOT, 'tests', 'golden', 'dataset')
CLASSES = [('table', '04379243', 7), ('car', '02958343', 13)]
N_POINTS = 64
FORMATS = ('ascii', 'binary_little_endian', 'binary_big_endian')
SIZES_TREE = osp.join(ROOT, 'tests', 'golden', 'dataset_sizes')
SIZES = (32, 47, 63)
SPLIT = (.85, .05, .10)


def write_tree(rng):
    if osp.isdir(TREE):
        shutil.rmtree(TREE)
    k = 0
    for _, syn, count in CLASSES:
        os.makedirs(osp.join(TREE, syn))
        for i in range(count):
            scale = np.array([rng.uniform(0.1, 0.5), rng.uniform(0.1, 0.5), rng.uniform(0.05, 0.3)])
            pts = ((rng.random((N_POINTS, 3)) - 0.5) * 2 * scale)
            fmt = FORMATS[k % 3]
            path = osp.join(TREE, syn, 'model%02d%s.ply' % (i, 'abcdef'[k % 6]))
            kw = {}
            if k % 4 == 1:
                kw = dict(comments=['made for the tests', 'second comment'], obj_info=['sampled uniformly'])
            if k == 4:          # double coordinates (little endian), not representable in float32
                write_ply(path, [vertex(pts, 'double')], fmt, **kw)
            elif k == 8:        # colours between x and y (big endian)
                col = rng.integers(0, 256, (N_POINTS, 3))
                write_ply(path, [vertex(pts.astype(np.float32), 'float',
                                        extra_between=[('red', 'uchar', col[:, 0]), ('green', 'uchar', col[:, 1])],
                                        extra_after=[('blue', 'uchar', col[:, 2])])], fmt, **kw)
            elif k == 9:        # normals before x (ascii)
                nrm = rng.standard_normal((N_POINTS, 3)).astype(np.float32)
                write_ply(path, [vertex(pts.astype(np.float32), 'float32',
                                        extra_before=[('nx', 'float', nrm[:, 0]), ('ny', 'float', nrm[:, 1]), ('nz', 'float', nrm[:, 2])])],
                          fmt, **kw)
            elif k in (10, 12):  # a face element after vertex (little endian / ascii)
                faces = [rng.integers(0, N_POINTS, 3 + (j % 2)) for j in range(5)]
                write_ply(path, [vertex(pts.astype(np.float32)),
                                 ('face', [('vertex_indices', ('list', 'uchar', 'int'), faces)])], fmt, **kw)
            else:
                write_ply(path, [vertex(pts.astype(np.float32))], fmt, **kw)
            k += 1


def sort_axes_clouds(rng):
    pcs = np.empty((64, N_POINTS, 3), np.float32)
    for i in range(64):
        scale = np.array([rng.uniform(0.05, 0.5), rng.uniform(0.05, 0.5), rng.uniform(0.05, 0.5)])
        pcs[i] = ((rng.random((N_POINTS, 3)) - 0.5) * 2 * scale + rng.uniform(-0.2, 0.2, 3)).astype(np.float32)

    def box(i, lo, hi):
        pcs[i] = (rng.random((N_POINTS, 3)) * (np.array(hi) - np.array(lo)) + np.array(lo)).astype(np.float32)
        pcs[i, 0], pcs[i, 1] = np.float32(lo), np.float32(hi)          # the extremes are attained exactly
    box(0, [-0.5, -0.25, -0.125], [0.5, 0.25, 0.125])                   # x longer
    box(1, [-0.25, -0.5, -0.125], [0.25, 0.5, 0.125])                   # y longer
    box(2, [-0.25, 0.125, -0.125], [0.5, 0.875, 0.125])                 # x and y extents exactly equal (0.75)
    box(3, [-0.25, -0.125, -0.5], [0.25, 0.125, 0.5])                   # z longest, x > y
    box(4, [-0.125, -0.25, -0.5], [0.125, 0.25, 0.5])                   # z longest, y > x
    pcs[5] = np.float32([0.3, -0.2, 0.1])                               # one repeated point: every extent 0
    box(6, [-0.75, -1.0, -0.5], [-0.5, -0.25, -0.25])                   # negative coordinates only, y longer
    box(7, [-0.25, 0.125, -0.125], [0.25, 0.125, 0.125])                # y extent 0, x > 0
    box(8, [0.125, -0.25, -0.125], [0.125, 0.25, 0.125])                # x extent 0, y > 0
    box(9, [-0.25, -0.5, -0.125], [0.25, 0.5, 0.125])                   # y longer, with exact zeros in both x and y (-> -0.0)
    pcs[9, 5:9, 0] = 0.0
    pcs[9, 7:12, 1] = 0.0
    assert np.float32(0.5) - np.float32(-0.25) == np.float32(0.875) - np.float32(0.125)
    return pcs


def documented_sort_axes(pc, neg_rot):
    """The project's rule for ONE cloud, used only where the reference asserts."""
    ext = pc.max(axis=0) - pc.min(axis=0)
    swap, flip = ext[0] <= ext[1], ext[0] < ext[1]
    idx = np.array([1, 0, 2] if swap else [0, 1, 2])
    out = pc[:, idx].copy()
    if flip:
        out[:, int(neg_rot)] = -out[:, int(neg_rot)]
    return out, idx


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--reference', required=True, help='checkout of the reference project')
    ref = ap.parse_args().reference
    sys.modules.setdefault('tensorflow', types.ModuleType('tensorflow'))
    try:
        import six  # noqa: F401
    except ImportError:                                   # what in_out.py takes from six
        six = types.ModuleType('six')
        six.iteritems = lambda d: iter(d.items())
        moves = types.ModuleType('six.moves')
        import pickle
        moves.cPickle = pickle
        six.moves = moves
        sys.modules.update({'six': six, 'six.moves': moves, 'six.moves.cPickle': pickle})
    sys.path.insert(0, ref)
    from src import in_out as R
    from src import shift_rotate_util as S

    rng = np.random.default_rng(20)
    write_tree(rng)
    out = {}
    for _, syn, _ in CLASSES:
        for name in sorted(os.listdir(osp.join(TREE, syn))):
            out['ply__%s__%s' % (syn, name[:-4])] = R.load_ply(osp.join(TREE, syn, name))

    # drawn from a generator of their own, so that the files and arrays above stay what they were
    rng_sizes = np.random.default_rng(21)
    if osp.isdir(SIZES_TREE):
        shutil.rmtree(SIZES_TREE)
    os.makedirs(SIZES_TREE)
    for count, fmt in zip(SIZES, FORMATS):
        pts = ((rng_sizes.random((count, 3)) - 0.5) * 0.8).astype(np.float32)
        path = osp.join(SIZES_TREE, 'points%02d.ply' % count)
        write_ply(path, [vertex(pts)], fmt, comments=['%d points' % count])
        out['sizes__points%02d' % count] = R.load_ply(path)

    for n in (7, 13, 20, 4379):
        tr, va, te, perm = R.split_data(np.arange(n) * 3 + 1, SPLIT, 42)
        out.update({'split%d_train' % n: tr, 'split%d_val' % n: va, 'split%d_test' % n: te, 'split%d_perm' % n: perm})

    walk = R.files_in_subdirs
    R.files_in_subdirs = lambda top_dir, pattern: iter(sorted(walk(top_dir, pattern)))
    for set_type in ('train_set', 'val_set', 'test_set'):
        ds, slice_idx, pc_label = R.load_dataset([c[0] for c in CLASSES], set_type, TREE)
        out[set_type + '_pc'] = ds.point_clouds
        out[set_type + '_labels'] = np.atleast_1d(ds.labels).astype(str)
        out[set_type + '_slice_idx'] = np.array(slice_idx)
        out[set_type + '_pc_label'] = np.array(pc_label).astype(np.int8)
        out[set_type + '_sorted'] = S.sort_axes(ds.point_clouds.copy()) if len(ds.point_clouds) else ds.point_clouds.copy()

    pcs = sort_axes_clouds(rng)
    accepts = np.ones(len(pcs), bool)
    res = {0: np.empty_like(pcs), 1: np.empty_like(pcs)}
    idx = np.empty((len(pcs), 3), np.int32)
    for i in range(len(pcs)):
        try:
            for neg in (0, 1):
                res[neg][i] = S.sort_axes(pcs[i:i + 1].copy(), neg_rot=bool(neg))[0]
            idx[i] = S.get_sort_axes_idx(pcs[i:i + 1].copy())[0][0]
        except AssertionError:
            accepts[i] = False
            for neg in (0, 1):
                res[neg][i], idx[i] = documented_sort_axes(pcs[i], neg)
    assert list(np.flatnonzero(~accepts)) == [5, 7, 8], np.flatnonzero(~accepts)
    assert list(idx[2]) == [1, 0, 2] and np.array_equal(res[1][2], pcs[2][:, [1, 0, 2]])      # the tie: swapped, not negated
    # the whole accepted batch at once gives the same as cloud by cloud
    for neg in (0, 1):
        assert np.array_equal(S.sort_axes(pcs[accepts].copy(), neg_rot=bool(neg)).view(np.uint32), res[neg][accepts].view(np.uint32))
    out.update(sa_in=pcs, sa_out_neg0=res[0], sa_out_neg1=res[1], sa_idx=idx, sa_ref_accepts=accepts)

    for n in (1, 2, 7, 17):
        ds = R.PointCloudDataSet(np.arange(n, dtype=np.float32).reshape(n, 1, 1), init_shuffle=False)
        out['shuffle55_%d' % n] = ds.shuffle_data(seed=55).point_clouds[:, 0, 0].astype(np.int64)
    ds = R.PointCloudDataSet(np.arange(7, dtype=np.float32).reshape(7, 1, 1), labels=np.arange(7), init_shuffle=False).shuffle_data(seed=55)
    out['next_batch_ids'] = np.stack([ds.next_batch(3)[0][:, 0, 0].astype(np.int64) for _ in range(4)])
    assert ds.epochs_completed == 1

    np.savez_compressed(osp.join(ROOT, 'tests', 'golden', 'dataset.npz'), **out)
    total = sum(osp.getsize(osp.join(d, f)) for d, _, fs in os.walk(TREE) for f in fs)
    print('wrote %d arrays; tree %d bytes, npz %d bytes' % (len(out), total, osp.getsize(osp.join(ROOT, 'tests', 'golden', 'dataset.npz'))))


if __name__ == '__main__':
    main()
