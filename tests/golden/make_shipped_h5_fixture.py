"""The reference's three shipped Keras .h5 files of the autoencoder path, as test fixtures for
tests/test_h5lite.py::test_reads_the_reference_shipped_files.

Stored as tests/golden/shipped_h5/<stem>.h5.xz with the data of every layer kernel and bias
zeroed in place, plus regions.json: for each file, where those arrays lie (found by searching
the file's bytes for the arrays of ae_path_weights.npz, each exactly once -- not by the reader
under test) and the SHA-256 of the whole file. The test writes the arrays back from
ae_path_weights.npz and checks the hash, so it reads the file byte for byte as shipped.
The one exception: the data of ae_emulator.h5's Adam moment slots (optimizer_weights/**/m:0
and v:0) stays zeroed -- the test reads the layers and the step counter, not the moments.
Run once:  python tests/golden/make_shipped_h5_fixture.py <reference>/VeryAccurateEmulator/models/autoencoder_based_emulator
Writes tests/golden/shipped_h5/{ae_emulator,encoder,decoder}.h5.xz and regions.json."""
import hashlib
import importlib
import json
import lzma
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))
h5 = importlib.import_module("21cmvae_amd.h5lite")


def moment_extents(path):
    """(file offset, bytes) of the contiguous data of every optimizer moment dataset."""
    out = []
    with h5.File(path) as f:
        ow = f["optimizer_weights"]
        for w in (h5._s(n) for n in np.atleast_1d(ow.attrs["weight_names"])):
            if w.endswith("/m:0") or w.endswith("/v:0"):
                d = ow[w]
                kind, off, size = d._data
                assert kind == "contig"
                n = int(np.prod(d.shape)) * np.dtype(d.dtype).itemsize
                assert size in (None, n)
                out.append((off + d._rd.base, n))
    return out


def main(src):
    dst = os.path.join(HERE, "shipped_h5")
    os.makedirs(dst, exist_ok=True)
    weights = np.load(os.path.join(HERE, "ae_path_weights.npz"))
    regions = {}
    for stem in ("ae_emulator", "encoder", "decoder"):
        p = os.path.join(src, stem + ".h5")
        buf = bytearray(open(p, "rb").read())
        if stem == "ae_emulator":
            for off, n in moment_extents(p):
                buf[off:off + n] = bytes(n)
        found = []
        for i in range(int(weights[stem + "/n_layers"])):
            for key in ("%s/W%d" % (stem, i), "%s/b%d" % (stem, i)):
                blob = np.ascontiguousarray(weights[key], "<f4").tobytes()
                off = buf.find(blob)
                assert off >= 0 and buf.find(blob, off + 1) < 0, "%s: not found exactly once in %s" % (key, p)
                found.append((key, off))
        regions[stem] = {"sha256": hashlib.sha256(bytes(buf)).hexdigest(), "size": len(buf), "arrays": found}
        for key, off in found:
            n = weights[key].nbytes
            buf[off:off + n] = bytes(n)
        with lzma.open(os.path.join(dst, stem + ".h5.xz"), "wb", preset=9 | lzma.PRESET_EXTREME) as f:
            f.write(bytes(buf))
    with open(os.path.join(dst, "regions.json"), "w") as f:
        json.dump(regions, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main(sys.argv[1])
