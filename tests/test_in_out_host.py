"""CPU: the dataset stage (geometric_adv_amd/in_out.py) against tests/golden/dataset.npz, which tools/make_golden_dataset.py
recorded from the reference's own src/in_out.py on the PLY tree tests/golden/dataset/ -- the project's PLY reader on every file
form, its refusals, the 85/5/10 split, load_dataset and PointCloudDataSet's shuffles."""
import os
import os.path as osp

import numpy as np
import pytest

from _ply_writer import vertex, write_ply

GOLDEN = osp.join(osp.dirname(osp.abspath(__file__)), "golden")
TREE = osp.join(GOLDEN, "dataset")
CLASSES = ["table", "car"]
SYNSETS = {"table": "04379243", "car": "02958343"}


@pytest.fixture(scope="module")
def golden():
    return np.load(osp.join(GOLDEN, "dataset.npz"))


def _tree_files():
    return sorted(osp.join(d, f) for d, _, fs in os.walk(TREE) for f in fs if f.endswith(".ply"))


def test_the_tree_has_every_file_form():
    files = _tree_files()
    assert len(files) == 20
    assert [len(os.listdir(osp.join(TREE, SYNSETS[c]))) for c in CLASSES] == [7, 13]
    heads = [open(f, "rb").read().split(b"end_header")[0] for f in files]
    for word in (b"format ascii", b"format binary_little_endian", b"format binary_big_endian", b"property double x",
                 b"property uchar red", b"property float nx", b"element face", b"comment ", b"obj_info "):
        assert any(word in h for h in heads), word


def test_every_golden_ply_file_loads_equal_to_the_reference(golden):
    from geometric_adv_amd import in_out
    seen_double = False
    for f in _tree_files():
        want = golden["ply__%s__%s" % (osp.basename(osp.dirname(f)), osp.basename(f)[:-4])]
        got = in_out.load_ply(f)
        assert got.dtype == np.float32 and got.shape == (64, 3)
        seen_double |= want.dtype == np.float64 and not np.array_equal(want, want.astype(np.float32))
        # the reference stores what it loads in a float32 array (in_out.py:174-180)
        assert np.array_equal(got.view(np.uint32), want.astype(np.float32).view(np.uint32)), f
    assert seen_double


def test_files_of_other_vertex_counts_load_equal_to_the_reference(golden):
    """The tree's files all hold 64 points (the folder loader needs one count); these hold 32, 47 and 63, one per format."""
    from geometric_adv_amd import in_out
    folder = osp.join(GOLDEN, "dataset_sizes")
    assert sorted(os.listdir(folder)) == ["points32.ply", "points47.ply", "points63.ply"]
    for count in (32, 47, 63):
        want = golden["sizes__points%02d" % count]
        got = in_out.load_ply(osp.join(folder, "points%02d.ply" % count))
        assert got.dtype == np.float32 and got.shape == (count, 3) == want.shape
        assert np.array_equal(got.view(np.uint32), want.astype(np.float32).view(np.uint32))
    # and the folder loader says which file does not fit
    files = [osp.join(folder, "points32.ply"), osp.join(folder, "points47.ply")]
    with pytest.raises(ValueError, match="points47.ply holds a cloud of shape"):
        in_out.load_point_clouds_from_filenames(files, 2, in_out.pc_loader)


def _pts(n=5):
    return (np.arange(3 * n, dtype=np.float32).reshape(n, 3) / 8 - 1).astype(np.float32)


@pytest.mark.parametrize("case, reason", [
    ("no_x", "no 'x' property"), ("no_z", "no 'z' property"), ("list_in_vertex", "list property inside the vertex"),
    ("list_before_vertex_binary", "before vertex in a binary file"), ("truncated_binary", "truncated body"),
    ("truncated_ascii", "truncated body"), ("short_ascii_row", "truncated body"), ("unknown_format", "unknown format"),
    ("no_format", "unknown format"), ("no_vertex", "no vertex element"), ("not_ply", "not a PLY file"),
    ("int_coordinates", "must be float or double")])
def test_load_ply_refuses_with_the_reason(tmp_path, case, reason):
    from geometric_adv_amd import in_out
    p, path = _pts(), str(tmp_path / "bad.ply")
    le = "binary_little_endian"
    if case == "no_x":
        write_ply(path, [("vertex", [("y", "float", p[:, 1]), ("z", "float", p[:, 2])])], le)
    elif case == "no_z":
        write_ply(path, [("vertex", [("x", "float", p[:, 0]), ("y", "float", p[:, 1])])], "ascii")
    elif case == "list_in_vertex":
        write_ply(path, [vertex(p, extra_after=[("tags", ("list", "uchar", "int"), [[1, 2]] * len(p))])], le)
    elif case == "list_before_vertex_binary":
        write_ply(path, [("face", [("vertex_indices", ("list", "uchar", "int"), [[0, 1, 2]])]), vertex(p)], le)
    elif case == "truncated_binary":
        write_ply(path, [vertex(p)], "binary_big_endian", truncate=1)
    elif case == "truncated_ascii":
        write_ply(path, [vertex(p)], "ascii")
        lines = open(path, "rb").read().split(b"\n")
        open(path, "wb").write(b"\n".join(lines[:-2]) + b"\n")              # the last vertex line is gone
    elif case == "short_ascii_row":
        write_ply(path, [vertex(p)], "ascii")
        data = open(path, "rb").read().rstrip(b"\n")
        open(path, "wb").write(data[:data.rindex(b" ")] + b"\n")            # the last vertex has two values
    elif case == "unknown_format":
        write_ply(path, [vertex(p)], "binary_middle_endian")
    elif case == "no_format":
        write_ply(path, [vertex(p)], "ascii")
        data = open(path, "rb").read()
        open(path, "wb").write(data.replace(b"format ascii 1.0\n", b""))
    elif case == "no_vertex":
        write_ply(path, [("face", [("vertex_indices", ("list", "uchar", "int"), [[0, 1, 2]])])], "ascii")
    elif case == "not_ply":
        open(path, "wb").write(b"OFF\n3 0 0\n")
    elif case == "int_coordinates":
        write_ply(path, [vertex(p * 8, "int")], le)
    with pytest.raises(ValueError, match=reason):
        in_out.load_ply(path)


def test_load_ply_accepts_what_the_refusals_border_on(tmp_path):
    """A list element BEFORE vertex is fine in an ascii file (one line per entry), scalar elements before vertex are skipped
    in a binary one, and CRLF header lines are read."""
    from geometric_adv_amd import in_out
    p = _pts()
    face = ("face", [("vertex_indices", ("list", "uchar", "int"), [[0, 1, 2], [1, 2, 3, 4]])])
    write_ply(str(tmp_path / "a.ply"), [face, vertex(p)], "ascii")
    assert np.array_equal(in_out.load_ply(str(tmp_path / "a.ply")), p)
    cam = ("camera", [("fx", "double", [1.5, 2.5]), ("id", "short", [3, 4])])
    for fmt in ("binary_little_endian", "binary_big_endian"):
        write_ply(str(tmp_path / "b.ply"), [cam, vertex(p, "double")], fmt)
        assert np.array_equal(in_out.load_ply(str(tmp_path / "b.ply")), p)
    write_ply(str(tmp_path / "c.ply"), [vertex(p)], "binary_little_endian", comments=["x"])
    head, body = open(str(tmp_path / "c.ply"), "rb").read().split(b"end_header\n")
    open(str(tmp_path / "c.ply"), "wb").write(head.replace(b"\n", b"\r\n") + b"end_header\r\n" + body)
    assert np.array_equal(in_out.load_ply(str(tmp_path / "c.ply")), p)


def test_synset_table_inverts():
    from geometric_adv_amd import in_out
    table = in_out.snc_category_to_synth_id()
    assert len(table) == 57 and table["table"] == "04379243" and table["car"] == "02958343" and table["chair"] == "03001627"
    assert all(in_out.snc_synth_id_to_category[v] == k for k, v in table.items())


@pytest.mark.parametrize("n", [7, 13, 20, 4379])
def test_split_data_is_the_reference_split(golden, n):
    from geometric_adv_amd import in_out
    data = np.arange(n) * 3 + 1
    tr, va, te, perm = in_out.split_data(data, (.85, .05, .10), 42)
    for got, key in ((tr, "train"), (va, "val"), (te, "test"), (perm, "perm")):
        assert np.array_equal(got, golden["split%d_%s" % (n, key)]), key
    assert len(tr) == int(.85 * n + 0.5) and len(tr) + len(va) == int((.85 + .05) * n + 0.5)
    # a given perm is reused as it is, whatever the seed
    tr2, va2, te2, perm2 = in_out.split_data(data[::-1].copy(), (.85, .05, .10), 7, perm)
    assert perm2 is perm and np.array_equal(np.concatenate([tr2, va2, te2]), data[::-1][perm])


@pytest.mark.parametrize("set_type", ["train_set", "val_set", "test_set"])
def test_load_dataset_is_the_reference_on_sorted_files(golden, set_type):
    from geometric_adv_amd import in_out
    ds, slice_idx, pc_label = in_out.load_dataset(CLASSES, set_type, TREE)
    assert ds.point_clouds.dtype == np.float32
    assert np.array_equal(ds.point_clouds.view(np.uint32), golden[set_type + "_pc"].view(np.uint32))
    assert list(np.atleast_1d(ds.labels).astype(str)) == list(golden[set_type + "_labels"])
    assert list(slice_idx) == list(golden[set_type + "_slice_idx"])
    assert list(pc_label) == list(golden[set_type + "_pc_label"])
    assert ds.num_examples == len(golden[set_type + "_pc"]) == {"train_set": 17, "val_set": 1, "test_set": 2}[set_type]


def test_walk_order_returns_the_same_files():
    from geometric_adv_amd import in_out
    walk = list(in_out.files_in_subdirs(TREE, ".ply", file_order="walk"))
    assert sorted(walk) == list(in_out.files_in_subdirs(TREE, ".ply")) == _tree_files()
    a = in_out.load_all_point_clouds_under_folder(osp.join(TREE, SYNSETS["car"]), n_threads=8, file_order="walk")
    b = in_out.load_all_point_clouds_under_folder(osp.join(TREE, SYNSETS["car"]), n_threads=8)
    assert sorted(a.labels) == list(b.labels) and a.num_examples == 13
    order = [list(a.labels).index(lbl) for lbl in b.labels]
    assert np.array_equal(a.point_clouds[order], b.point_clouds)
    with pytest.raises(ValueError):
        list(in_out.files_in_subdirs(TREE, ".ply", file_order="random"))


def test_reading_threads_are_capped():
    from geometric_adv_amd import in_out
    assert in_out.MAX_READ_THREADS == 8
    pcs, models, syn = in_out.load_point_clouds_from_filenames(_tree_files()[:3], 10 ** 6, in_out.pc_loader)
    assert pcs.shape == (3, 64, 3) and list(syn) == ["02958343"] * 3


def _ids(n):
    return np.arange(n, dtype=np.float32).reshape(n, 1, 1)


@pytest.mark.parametrize("n", [1, 2, 7, 17])
def test_shuffle_data_55_is_the_reference_order(golden, n):
    from geometric_adv_amd import in_out
    ds = in_out.PointCloudDataSet(_ids(n), labels=np.arange(n), init_shuffle=False).shuffle_data(seed=55)
    assert list(ds.point_clouds[:, 0, 0].astype(int)) == list(golden["shuffle55_%d" % n])
    assert list(ds.labels) == list(golden["shuffle55_%d" % n])


def test_next_batch_wraps_around_and_reshuffles(golden):
    from geometric_adv_amd import in_out
    ds = in_out.PointCloudDataSet(_ids(7), labels=np.arange(7), init_shuffle=False).shuffle_data(seed=55)
    got = []
    for k in range(4):
        pcs, labels, noisy = ds.next_batch(3)
        assert noisy is None and list(labels) == list(pcs[:, 0, 0].astype(int))
        got.append(pcs[:, 0, 0].astype(int))
        assert ds.epochs_completed == (0 if k < 2 else 1)
    want = golden["next_batch_ids"]
    assert np.array_equal(np.stack(got), want)
    assert list(want[0]) + list(want[1]) == list(golden["shuffle55_7"][:6])       # two batches of the first order ...
    assert len(set(want[2]) | set(want[3])) == 6                                  # ... then two of a fresh one


def test_merge_full_epoch_and_shuffle_points():
    from geometric_adv_amd import in_out
    a = in_out.PointCloudDataSet(_ids(3), labels=np.array(["a0", "a1", "a2"], dtype=object), init_shuffle=False)
    b = in_out.PointCloudDataSet(_ids(2) + 10, labels=np.array(["b0", "b1"], dtype=object), init_shuffle=False)
    a.next_batch(2)
    m = a.merge(b)
    assert m is a and a.num_examples == 5 and a._cursor == 0
    assert list(a.labels) == ["a0", "a1", "a2", "b0", "b1"] and list(a.point_clouds[:, 0, 0]) == [0, 1, 2, 10, 11]
    pcs, labels, noisy = a.full_epoch_data(shuffle=True, seed=3)
    np.random.seed(3)
    perm = np.arange(5)
    np.random.shuffle(perm)
    assert list(pcs[:, 0, 0]) == list(a.point_clouds[perm, 0, 0]) and list(labels) == list(a.labels[perm]) and noisy is None
    assert list(a.full_epoch_data(shuffle=False)[0][:, 0, 0]) == [0, 1, 2, 10, 11]
    pts = np.arange(2 * 6 * 3, dtype=np.float32).reshape(2, 6, 3)
    ds = in_out.PointCloudDataSet(pts, init_shuffle=False).shuffle_points(seed=9)
    np.random.seed(9)
    perm = np.arange(6)
    for i in range(2):
        np.random.shuffle(perm)
        assert np.array_equal(ds.point_clouds[i], pts[i, perm])
    assert list(ds.labels) == [1, 1] and ds.labels.dtype == np.int8


def test_a_merged_set_of_one_example_can_be_shuffled():
    """An empty class split merged with a one-cloud split (the golden tree's validation set): the labels keep their axis, so
    shuffle_data and next_batch work where the reference's squeezed 0-d labels fail."""
    from geometric_adv_amd import in_out
    ds, slice_idx, pc_label = in_out.load_dataset(CLASSES, "val_set", TREE)
    assert ds.num_examples == 1 and ds.labels.shape == (1,) and slice_idx == [0, 0, 1] and pc_label == [1]
    ds.shuffle_data(seed=55)
    pcs, labels, _ = ds.next_batch(4)
    assert pcs.shape == (1, 64, 3) and labels.shape == (1,) and str(labels[0]).startswith("02958343_model")
