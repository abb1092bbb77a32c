"""CPU: the host side of train.run_train -- the training stream (data.DescriptorStream = train.py's ``repeat().batch(B)``) and the
validation batching (data.validation_descriptors = ``repeat(2).batch(B).take(n)``) against what the reference's own generator yields
(tests/golden/make_train_stream_golden.py), exact resume of the stream, MetricHistory, resolve_weight_selector, the AW- rule, the
best / last weight files and the command line."""
import json
import os

import numpy as np
import pytest

from tests import util

G = os.path.join(util.ROOT, "tests", "golden")
FLIP = [5, 4, 3, 2, 1, 0, 6, 7, 8, 9, 10, 16, 15, 14, 13, 12, 11]
MODES = {
    "list": dict(seq_len=27, stride=3, padding_type="copy", mask_stride=[3, 9, 15], rand_shift_stride_mask=True, flip_augment=True,
                 in_batch_augment=False, shuffle=True, subsample=4),
    "inbatch": dict(seq_len=9, stride=1, padding_type="zeros", mask_stride=[2, 4], rand_shift_stride_mask=True, flip_augment=True,
                    in_batch_augment=True, shuffle=True, subsample=5),
    "val": dict(seq_len=27, stride=3, padding_type="copy", mask_stride=9, flip_augment=False, shuffle=False, subsample=4),
}


def _golden():
    return np.load(os.path.join(G, "train_stream_expected.npz"))


def _generator(tag, g):
    from uplift_upsample_3dhpe_amd import data as D
    n = len(g["lens"])
    table = D.PoseTable([g[f"video2d_{v}"] for v in range(n)], [g[f"video3d_{v}"] for v in range(n)], subjects=g["subjects"],
                        actions=g["actions"], frame_rates=g["rates"], device="cpu")
    return D.SequenceGenerator(table, flip_lr_indices=FLIP, target_frame_rate=50, seed=7, **MODES[tag])


def stride_masks(desc, seq_len):
    """The stride mask a descriptor stands for (uu3d_gather_windows: token n is kept when ((n - N // 2) * stride + shift) % abs mask
    stride == 0)."""
    d = np.asarray(desc, np.int64)
    n = np.arange(seq_len)[None, :]
    return (np.mod((n - seq_len // 2) * d[:, 2:3] + d[:, 4:5], d[:, 3:4]) == 0).astype(np.uint8)


def _check_rows(g, tag, desc, seq_len, rows=slice(None)):
    assert np.array_equal(desc[:, 0], g[f"{tag}/video"][rows])
    assert np.array_equal(desc[:, 1], g[f"{tag}/index"][rows])
    assert np.array_equal(desc[:, 5], g[f"{tag}/flip"][rows])
    assert np.array_equal(stride_masks(desc, seq_len), g[f"{tag}/stride_mask"][rows])


@pytest.mark.parametrize("tag", ["list", "inbatch"])
def test_training_stream_matches_the_reference_across_generator_epochs(tag):
    from uplift_upsample_3dhpe_amd.data import DescriptorStream
    g = _golden()
    B, per_epoch = int(g[f"{tag}/batch"]), int(g[f"{tag}/windows_per_epoch"])
    n_batches = len(g[f"{tag}/index"]) // B
    assert n_batches * B > 2 * per_epoch and per_epoch % B != 0      # at least two boundaries, inside batches
    stream = DescriptorStream(_generator(tag, g), B)
    desc = []
    for _ in range(n_batches):
        d, cams = stream.next()
        assert d.shape == (B, 6) and d.dtype == np.int32 and cams is None
        desc.append(d)
    _check_rows(g, tag, np.concatenate(desc), MODES[tag]["seq_len"])
    assert stream.epochs == -(-n_batches * B // per_epoch)


def test_validation_batches_wrap_like_repeat_two_take():
    from uplift_upsample_3dhpe_amd.data import validation_descriptors
    g = _golden()
    B = int(g["val/batch"])
    gen = _generator("val", g)
    desc, cams, n_batches, examples = validation_descriptors(gen, B, -1)
    assert examples == int(g["val/examples"]) == len(gen) and cams is None
    assert n_batches == -(-examples // B) and len(desc) == n_batches * B > examples
    _check_rows(g, "val", desc, MODES["val"]["seq_len"])
    assert np.array_equal(desc[examples:], desc[:len(desc) - examples])            # the last batch wraps to the first windows
    d2, _, n2, e2 = validation_descriptors(gen, B, 20)                               # a VALIDATION_EXAMPLES below the window count
    assert (n2, e2) == (2, 20) and np.array_equal(d2, desc[:32])
    with pytest.raises(ValueError):
        validation_descriptors(gen, B, len(gen) + 1)


@pytest.mark.parametrize("tag,cut", [("list", 3), ("list", 4), ("inbatch", 7), ("inbatch", 1)])
def test_stream_state_restores_mid_epoch(tag, cut):
    """A stream saved after ``cut`` batches (inside a generator epoch, or right after a batch that straddled two) and loaded into a
    fresh generator continues with the same batches as the uninterrupted one."""
    from uplift_upsample_3dhpe_amd.data import DescriptorStream
    g = _golden()
    B = int(g[f"{tag}/batch"])
    a = DescriptorStream(_generator(tag, g), B)
    for _ in range(cut):
        a.next()
    sd = json.loads(json.dumps(a.state_dict()))                                      # what a checkpoint stores
    ref = [a.next()[0] for _ in range(6)]
    b = DescriptorStream(_generator(tag, g), B)
    b.load_state_dict(sd)
    got = [b.next()[0] for _ in range(6)]
    assert all(np.array_equal(x, y) for x, y in zip(ref, got))
    assert (a.epochs, a.offset) == (b.epochs, b.offset)
    fresh = DescriptorStream(_generator(tag, g), B)                                  # the state of a stream that has not started
    fresh.load_state_dict(json.loads(json.dumps(DescriptorStream(_generator(tag, g), B).state_dict())))
    assert np.array_equal(fresh.next()[0], DescriptorStream(_generator(tag, g), B).next()[0])


def test_metric_history():
    from uplift_upsample_3dhpe_amd.utils.metric_history import MetricHistory
    h = MetricHistory()
    h.add_metric("loss", higher_is_better=False)
    h.add_metric("acc", higher_is_better=True)
    with pytest.raises(AssertionError):
        h.add_metric("loss")
    assert h.best_value("loss") == (None, None) and h.latest_value("loss") is None and h.value_at_step("loss", 1) is None
    for step, (l, a) in zip([2, 4, 6, 8], [(0.5, 1.0), (0.3, 3.0), (0.3, 2.0), (0.4, 3.0)]):
        h.add_data("loss", l, step)
        h.add_data("acc", a, step)
    assert h.best_value("loss") == (0.3, 4)                  # first of equal bests
    assert h.best_value("acc") == (3.0, 4)
    assert h.value_at_step("acc", 6) == 2.0 and h.value_at_step("acc", 5) is None
    assert h.latest_value("loss") == 0.4
    lines = []
    h.print_all_for_best_metric("loss", log=lines.append)
    assert lines == ["loss: 0.3 (step 4)", "acc: 3.000 (step 4)"]
    lines = []
    h.print_best(log=lines.append)
    assert lines == ["loss: 0.3 (step 4)", "acc: 3.000 (step 4)"]
    h2 = MetricHistory.from_state_dict(json.loads(json.dumps(h.state_dict())))
    assert h2.history == h.history and h2.metrics == h.metrics and h2.higher == h.higher


def test_resolve_weight_selector(tmp_path):
    from uplift_upsample_3dhpe_amd.utils.weight_io import resolve_weight_selector
    assert resolve_weight_selector(None) is None
    assert resolve_weight_selector("no/such/dir/w.h5") == "no/such/dir/w.h5"          # an extension: taken as it is
    for name in ["best_weights_0090.h5", "best_weights_0012.h5", "best_weights_0005.npz", "last_weights_0001.h5"]:
        (tmp_path / name).write_bytes(b"")
    assert resolve_weight_selector(str(tmp_path / "best_weights")) == str(tmp_path / "best_weights_0012.h5")
    assert resolve_weight_selector(str(tmp_path / "last")) == str(tmp_path / "last_weights_0001.h5")
    with pytest.raises(FileNotFoundError):
        resolve_weight_selector(str(tmp_path / "cp"))


def test_aw_prefix_rule_and_metrics():
    from uplift_upsample_3dhpe_amd import train as T
    assert T.best_checkpoint_metric("AW-MPJPE", "h36m") == "AW-MPJPE"
    assert T.best_checkpoint_metric("AW-MPJPE", "amass") == "MPJPE"
    assert T.best_checkpoint_metric("PAMPJPE", "amass") == "PAMPJPE"
    assert T.best_checkpoint_metric(None, "amass") is None
    assert T.validation_metrics(True) == ["loss", "MPJPE", "NMPJPE", "PAMPJPE", "AW-MPJPE", "AW-NMPJPE", "AW-PAMPJPE"]
    assert T.validation_metrics(False) == ["loss", "MPJPE", "NMPJPE", "PAMPJPE"]


def test_weight_files_replace_the_previous_one(tmp_path):
    from uplift_upsample_3dhpe_amd import train as T

    class Saver(object):
        def save_weights(self, path):
            with open(path, "w") as fh:
                fh.write("w")
    m = Saver()
    prev = None
    for epoch in (1, 2, 5):
        prev = T.replace_weight_file(m, str(tmp_path), "best", epoch, prev)
        assert os.path.basename(prev) == f"best_weights_{epoch:04d}.h5"
    last = T.replace_weight_file(m, str(tmp_path), "last", 12, None)
    assert sorted(os.listdir(tmp_path)) == ["best_weights_0005.h5", "last_weights_0012.h5"] and last.endswith("last_weights_0012.h5")
    for e in (3, 11, 7):
        np.savez(str(tmp_path / f"cp_{e:04d}.npz"), a=np.zeros(1))
    path, epoch = T.latest_checkpoint(str(tmp_path))
    assert epoch == 11 and path.endswith("cp_0011.npz")
    assert T.latest_checkpoint(str(tmp_path / "none")) == (None, 0)


def test_cli_flags_and_defaults_equal_the_reference():
    """train.py:200-263: the same flags, defaults and clean-up."""
    from uplift_upsample_3dhpe_amd import train as T
    parser = T.build_parser()
    flags = {a.dest: a.default for a in parser._actions if a.dest != "help"}
    assert flags == {"config": None, "gpu_id": None, "dataset": "h36m", "dataset_val": None, "h36m_path": "./data/data_3d_h36m.npz",
                     "amass_path": None, "amass_frame_rate": "50", "dataset_2d_path": "./data/data_2d_h36m_cpn_ft_h36m_dbb.npz",
                     "train_subset": "train", "val_subset": "val", "test_subset": None, "weights": None, "continue_training": False,
                     "out_dir": None}
    assert [a.dest for a in parser._actions if a.required] == ["out_dir"]
    with pytest.raises(SystemExit):
        T.parse_args([])
    a = T.parse_args(["--out_dir", "o", "--val_subset", "none", "--test_subset", "S9", "--continue_training", "True",
                      "--dataset", "AMASS", "--dataset_val", "H36M", "--amass_frame_rate", "25"])
    assert (a.val_subset, a.test_subset, a.continue_training, a.dataset, a.dataset_val, a.amass_frame_rate) == \
        (None, "S9", True, "amass", "h36m", 25)
    for off in ("False", "false", "f", "n", "0"):
        assert T.parse_args(["--out_dir", "o", "--continue_training", off]).continue_training is False
    assert T.parse_args(["--out_dir", "o", "--val_subset", ""]).val_subset is None
