"""CPU: the host side of train_ae / tst_ae -- configuration.json written and read back, the eight file names of the eval
folder, and the train_ae command line (the old form unchanged, the new flags, the refusal when no data source is given)."""
import json
import os.path as osp

import pytest


def test_configuration_round_trip(tmp_path):
    from geometric_adv_amd import train_ae
    flags = train_ae.parse_flags(["--data_dir", "somewhere", "--train_folder", str(tmp_path / "ae"), "--class_names", "chair", "lamp",
                                  "--sort_axes", "0", "--training_epochs", "7", "--batch_size", "4", "--held_out_step", "2"])
    conf = train_ae.make_configuration(flags, 64)
    train_ae.save_configuration(flags.train_folder, conf)
    assert osp.exists(osp.join(flags.train_folder, "configuration.json"))
    back = train_ae.load_configuration(flags.train_folder)
    assert back == conf
    assert back == {"n_input": [64, 3], "loss": "chamfer", "batch_size": 4, "learning_rate": 0.0005, "training_epochs": 7,
                    "saver_step": 50, "bneck_size": 128, "object_class": ["2l"], "class_names": ["chair", "lamp"], "sort_axes": 0,
                    "experiment_name": "autoencoder", "held_out_step": 2, "data_source": "data_dir"}
    # a file that lacks a field is refused with the field's name
    del conf["class_names"]
    with open(osp.join(flags.train_folder, "configuration.json"), "w") as f:
        json.dump(conf, f)
    with pytest.raises(ValueError, match="class_names"):
        train_ae.load_configuration(flags.train_folder)


def test_default_configuration_is_the_reference_s():
    from geometric_adv_amd import train_ae
    conf = train_ae.make_configuration(train_ae.parse_flags(["--data_dir", "d"]), 2048)
    assert conf["object_class"] == ["13l"] and conf["sort_axes"] == 1 and conf["n_input"] == [2048, 3]
    assert conf["class_names"] == ['table', 'car', 'chair', 'airplane', 'sofa', 'rifle', 'lamp', 'watercraft', 'bench', 'loudspeaker',
                                   'cabinet', 'display', 'telephone']
    assert (conf["batch_size"], conf["learning_rate"], conf["training_epochs"], conf["saver_step"], conf["held_out_step"]) == \
        (50, 0.0005, 500, 50, 5)


def test_save_config_and_exit_needs_no_gpu(tmp_path):
    import numpy as np
    from geometric_adv_amd import train_ae
    np.save(tmp_path / "clouds.npy", np.zeros((3, 128, 3), np.float32))
    out = train_ae.main(["--train_data", str(tmp_path / "clouds.npy"), "--train_folder", str(tmp_path / "ae"),
                         "--save_config_and_exit", "1"])
    assert out == []
    conf = train_ae.load_configuration(str(tmp_path / "ae"))
    assert conf["n_input"] == [128, 3]
    # a .npy of clouds says nothing about classes or axes: nothing is claimed
    assert (conf["data_source"], conf["class_names"], conf["object_class"], conf["sort_axes"]) == ("train_data", [], [], 0)
    golden_tree = osp.join(osp.dirname(osp.abspath(__file__)), "golden", "dataset")
    train_ae.main(["--data_dir", golden_tree, "--class_names", "car", "table", "--train_folder", str(tmp_path / "ae2"),
                   "--save_config_and_exit", "1"])
    conf = train_ae.load_configuration(str(tmp_path / "ae2"))
    assert conf["n_input"] == [64, 3] and conf["class_names"] == ["car", "table"] and conf["object_class"] == ["2l"]


def test_eval_file_names():
    from geometric_adv_amd import tst_ae
    assert tst_ae.eval_file_names("test_set", ["13l"]) == {
        "pc_classes": "pc_classes_13l.npy", "pc_label": "pc_label_test_set_13l.npy", "slice_idx": "slice_idx_test_set_13l.npy",
        "point_clouds": "point_clouds_test_set_13l.npy", "latent_vectors": "latent_vectors_test_set_13l.npy",
        "reconstructions": "reconstructions_test_set_13l.npy", "ae_loss": "ae_loss_test_set_13l.npy",
        "eval_stats": "eval_stats_test_set_13l.txt"}
    two = tst_ae.eval_file_names("train_set", ["chair", "table"])
    assert two["pc_classes"] == "pc_classes_chair_table.npy" and two["pc_label"] == "pc_label_train_set_chair_table.npy"
    assert two["ae_loss"] == "ae_loss_train_set_chair_table.npy" and two["eval_stats"] == "eval_stats_train_set_chair_table.txt"
    assert len(two) == 8


def test_tst_ae_parser_has_the_reference_flags():
    from geometric_adv_amd import tst_ae
    f = tst_ae.build_parser().parse_args([])
    assert (f.restore_epoch, f.set_type, f.train_folder, f.output_folder_name, f.top_dir, f.data_dir) == \
        (500, "test_set", "log/autoencoder_victim", "eval", ".", None)


def test_train_ae_parser_accepts_the_old_command_line_unchanged():
    from geometric_adv_amd import train_ae
    f = train_ae.parse_flags(["--train_data", "clouds.npy", "--train_folder", "log/autoencoder_victim", "--training_epochs", "500"])
    assert (f.train_data, f.train_folder, f.training_epochs, f.data_dir) == ("clouds.npy", "log/autoencoder_victim", 500, None)
    assert (f.batch_size, f.learning_rate, f.saver_step, f.seed) == (50, 0.0005, 50, 0)
    f = train_ae.parse_flags(["--data_dir", "data/shapenet"])
    assert f.train_data is None and f.sort_axes == 1 and f.save_config_and_exit == 0 and f.held_out_step == 5


def test_train_ae_parser_rejects_a_run_without_data(capsys):
    from geometric_adv_amd import train_ae
    with pytest.raises(SystemExit) as e:
        train_ae.parse_flags(["--train_folder", "x"])
    assert e.value.code == 2
    assert "--data_dir" in capsys.readouterr().err
    with pytest.raises(SystemExit) as e:
        train_ae.parse_flags(["--data_dir", "d", "--train_data", "c.npy"])
    assert e.value.code == 2
    assert "give one of them" in capsys.readouterr().err
