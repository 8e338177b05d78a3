"""Records tests/golden/agg_parent.npz: the raw float64 outputs of the aggregation entry points and of the scores on the cases of
tests/agg_bits_cases.py, as the library computes them on the MI355X.  Recorded from a library of the commit before the family
rules were stated once in csrc/kernels_agg.hpp (the C ABI is the same, so this tree's binding drives it);
tests/test_agg_bits_gpu.py asserts that the library still gives these bits.

    python tests/golden/make_agg_parent.py [output.npz] [--lib libdsmgp_hip.so of the parent commit]

Deterministic (counter-stream inputs, no timing, fixed archive timestamps): a second run writes the same file, byte for byte."""
import io
import os
import sys
import zipfile

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path[:0] = [os.path.dirname(os.path.dirname(HERE)), os.path.dirname(HERE)]

from deepstructuredmixtures_amd import hipabi  # noqa: E402
import agg_bits_cases as abc  # noqa: E402


def main(path):
    arrays = {}
    for name in abc.CASES:
        for key, a in abc.run(name).items():
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
    argv = sys.argv[1:]
    if "--lib" in argv:
        i = argv.index("--lib")
        hipabi.LIB_PATH = os.path.abspath(argv[i + 1])
        del argv[i:i + 2]
    main(argv[0] if argv else os.path.join(HERE, "agg_parent.npz"))
