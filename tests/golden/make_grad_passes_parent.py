"""Records tests/golden/grad_passes_parent.npz: the raw float64 outputs of the four hyper-parameter gradient entry points (the
gradient tables, the lpd outputs and the triple of work_gradients()) on the cases of tests/grad_passes_cases.py, as the library
computes them on the MI355X.  Recorded from the commit before the gradient passes were built from one contraction plan;
tests/test_grad_passes_bits_gpu.py asserts that the library still gives these bits.

    python tests/golden/make_grad_passes_parent.py [output.npz]

Deterministic (counter-stream inputs, no timing, fixed archive timestamps): a second run writes the same file, byte for byte."""
import io
import os
import sys
import zipfile

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path[:0] = [os.path.dirname(os.path.dirname(HERE)), os.path.dirname(HERE)]

import grad_passes_cases as gpc  # noqa: E402


def main(path):
    arrays = {}
    for name in gpc.CASES:
        for key, a in gpc.run(name).items():
            assert a.dtype == np.float64
            arrays[f"{name}/{key}"] = a
        print(name, flush=True)
    with zipfile.ZipFile(path, "w", zipfile.ZIP_DEFLATED) as z:
        for key in sorted(arrays):
            buf = io.BytesIO()
            np.lib.format.write_array(buf, arrays[key], allow_pickle=False)
            z.writestr(zipfile.ZipInfo(key + ".npy", date_time=(1980, 1, 1, 0, 0, 0)), buf.getvalue(), zipfile.ZIP_DEFLATED)
    print(f"{path}: {len(arrays)} arrays, {os.path.getsize(path)} bytes")


if __name__ == "__main__":
    main(sys.argv[1] if len(sys.argv) > 1 else os.path.join(HERE, "grad_passes_parent.npz"))
