"""Training-stream fixtures from the REFERENCE's own H36mSequenceGenerator.  Run in the build container:

    python tests/golden/make_train_stream_golden.py     # needs the reference checkout -> tests/golden/train_stream_expected.npz

As make_windows_golden.py does, the class definition is taken out of the reference file's AST at run time and executed (nothing of it
is stored in this repository).  Its ``next_epoch_iterator()`` is called again and again and the windows are cut into batches the way
train.py's ``dataset.repeat().batch(B)`` (training) and ``dataset.repeat(2).batch(B).take(ceil(VE / B))`` (validation) do.  Stored
per window: the video (subject ids are unique per video), the centre frame, the flip bit (read off the yielded 3D centre frame), the
stride mask, and float64 checksums of the 2D / 3D window.  tests/test_train_loop_cpu.py checks data.DescriptorStream and
data.validation_descriptors against it, tests/test_train_loop_gpu.py the gathered batches."""
import ast
import math
import os

import numpy as np

SRC = "/root/reference/common/dataset/uplifiting_dataset.py"
tree = ast.parse(open(SRC).read())
node = next(n for n in tree.body if isinstance(n, ast.ClassDef) and n.name == "H36mSequenceGenerator")
ns = {"np": np, "math": math}
exec(compile(ast.Module(body=[node], type_ignores=[]), SRC, "exec"), ns)
Gen = ns["H36mSequenceGenerator"]

HERE = os.path.dirname(os.path.abspath(__file__))
FLIP = [5, 4, 3, 2, 1, 0, 6, 7, 8, 9, 10, 16, 15, 14, 13, 12, 11]
LENS = (3, 40, 97, 26, 7)
RATES = [50, 100, 50, 100, 50]
rng = np.random.default_rng(21)
p2 = [rng.uniform(-1, 1, size=(n, 17, 2)).astype(np.float32) for n in LENS]
p3 = [rng.normal(0, 0.4, size=(n, 17, 3)).astype(np.float32) for n in LENS]
cams = [rng.normal(size=11).astype(np.float32) for _ in LENS]
subjects, actions = [1, 5, 6, 7, 8], [0, 3, 3, 14, 2]
JW = np.arange(1, 18, dtype=np.float64)[None, :, None] * np.array([1.0, 2.0, 3.0])[None, None, :]   # joint / coordinate weights

# train modes: the flip LIST mode (every window twice, shuffled apart) and the in-batch mode (flipped copy right after its window)
MODES = {
    "list": dict(seq_len=27, stride=3, padding_type="copy", mask_stride=[3, 9, 15], rand_shift_stride_mask=True, flip_augment=True,
                 in_batch_augment=False, shuffle=True, subsample=4, batch=24, batches=14),
    "inbatch": dict(seq_len=9, stride=1, padding_type="zeros", mask_stride=[2, 4], rand_shift_stride_mask=True, flip_augment=True,
                    in_batch_augment=True, shuffle=True, subsample=5, batch=20, batches=10),
    # validation: no shuffle, flip or shift; VALIDATION_EXAMPLES 50 of 47 + ... windows -> the last batch wraps
    "val": dict(seq_len=27, stride=3, padding_type="copy", mask_stride=9, flip_augment=False, shuffle=False, subsample=4,
                batch=16, examples=-1),
}


def record(seq3, seq2, stride_mask, subject, i):
    v = subjects.index(int(subject))
    c3 = seq3[seq3.shape[0] // 2].astype(np.float64)
    raw = p3[v][int(i)].astype(np.float64)
    flipped = np.concatenate([-raw[:, :1], raw[:, 1:]], -1)[FLIP]
    if np.array_equal(c3, raw):
        fl = 0
    else:
        assert np.array_equal(c3, flipped)
        fl = 1
    w2 = (seq2.astype(np.float64) * JW[..., :2]).sum()
    w3 = (seq3.astype(np.float64) * JW).sum()
    return v, int(i), fl, stride_mask.astype(np.uint8), w2, w3


out = {"lens": np.array(LENS), "rates": np.array(RATES), "subjects": np.array(subjects), "actions": np.array(actions)}
for v, (a, b) in enumerate(zip(p2, p3)):
    out[f"video2d_{v}"] = a
    out[f"video3d_{v}"] = b
for tag, mode in MODES.items():
    mode = dict(mode)
    B = mode.pop("batch")
    n_batches = mode.pop("batches", None)
    examples = mode.pop("examples", None)
    g = Gen(p3, p2, cams, subjects, actions, RATES, "train", flip_lr_indices=FLIP, seed=7, verbose=False, **mode)
    if examples is not None:                                   # repeat(2).batch(B).take(ceil(VE / B))
        examples = len(g) if examples < 0 else examples
        n_batches = int(np.ceil(examples / B))
        epochs = 2
    else:                                                      # repeat().batch(B): enough generator epochs for the batches
        epochs = int(np.ceil(n_batches * B / len(g))) + 1
    rows = []
    for _ in range(epochs):
        for seq3, seq2, mask, cam, subject, action, i, stride_mask in g.next_epoch_iterator():
            rows.append(record(seq3, seq2, stride_mask, subject, i))
    rows = rows[:n_batches * B]
    assert len(rows) == n_batches * B
    out[f"{tag}/video"] = np.array([r[0] for r in rows], np.int32)
    out[f"{tag}/index"] = np.array([r[1] for r in rows], np.int32)
    out[f"{tag}/flip"] = np.array([r[2] for r in rows], np.int32)
    out[f"{tag}/stride_mask"] = np.stack([r[3] for r in rows])
    out[f"{tag}/sum2d"] = np.array([r[4] for r in rows])
    out[f"{tag}/sum3d"] = np.array([r[5] for r in rows])
    out[f"{tag}/batch"] = np.int64(B)
    out[f"{tag}/windows_per_epoch"] = np.int64(len(g))
    if examples is not None:
        out[f"{tag}/examples"] = np.int64(examples)
    print(tag, len(g), "windows per epoch,", n_batches, "batches of", B)
np.savez_compressed(os.path.join(HERE, "train_stream_expected.npz"), **out)
