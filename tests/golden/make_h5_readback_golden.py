"""What a REAL HDF5 library (h5py / libhdf5) reads back from the model-sized .h5 files the package writes:

    python tests/golden/make_h5_readback_golden.py PYTHON_WITH_H5PY      -> tests/golden/h5_readback_expected.json

For every case of tests/test_h5_cpu.py::test_model_sized_roundtrip_and_h5py_reads_our_files the file is written with
weight_io.save_keras_h5 (this interpreter), then read by h5py in PYTHON_WITH_H5PY (the main interpreter has no h5py):
the number of weight elements and the float64 sum of their absolute values, beside the sha256 of the file's bytes.
The test writes the same file again and checks it is byte for byte the one h5py read.
"""
import hashlib
import json
import os
import subprocess
import sys
import tempfile

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)

from tests import test_h5_cpu as T  # noqa: E402

READ = ("import h5py, numpy as np, sys\n"
        "f = h5py.File(sys.argv[1], 'r'); n = 0; s = 0.0\n"
        "for l in f.attrs['layer_names']:\n"
        "    g = f[l.decode()]\n"
        "    for wn in g.attrs['weight_names']:\n"
        "        a = np.asarray(g[wn.decode()]); n += a.size; s += float(np.abs(a.astype(np.float64)).sum())\n"
        "print(n, repr(s))\n")


def main(h5py_python):
    out = {}
    with tempfile.TemporaryDirectory() as d:
        for cfgname in T.ROUNDTRIP_CASES:
            path = os.path.join(d, cfgname + ".h5")
            T.write_model_h5(cfgname, path)
            n, s = subprocess.run([h5py_python, "-c", READ, path], capture_output=True, text=True, check=True).stdout.split()
            out[cfgname] = {"sha256": hashlib.sha256(open(path, "rb").read()).hexdigest(), "h5py_elements": int(n), "h5py_abs_sum": float(s)}
    with open(os.path.join(HERE, "h5_readback_expected.json"), "w") as f:
        json.dump(out, f, indent=1, sort_keys=True)
        f.write("\n")
    print(json.dumps(out, indent=1))


if __name__ == "__main__":
    if len(sys.argv) != 2:
        raise SystemExit(__doc__)
    main(sys.argv[1])
