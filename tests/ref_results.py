"""The answers of the reference's own code (oracle/_ref/, compiled from the reference tree, which a checkout does not
have), stored as fixtures under tests/golden/ so that the tests that compare against them stand alone.

A test asks `RefResults(name).get(call, inputs, live)`: the key is the call's name and a hash of its inputs, the value
the tuple of arrays / strings / numbers `live(lib)` returned when the fixtures were recorded.  To record them again,
with oracle/_ref built:

    SMK_REF_RECORD=1 python -m pytest tests/test_ref_sparse.py tests/test_hierclust.py -m "not gpu"
"""
import atexit
import ctypes as C
import hashlib
import os

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
RECORD = os.environ.get("SMK_REF_RECORD") == "1"


def _key(call, inputs):
    h = hashlib.sha1(call.encode())
    for x in inputs:
        if isinstance(x, np.ndarray):
            h.update(f"{x.dtype.str}{x.shape}".encode())
            h.update(np.ascontiguousarray(x).tobytes())
        else:
            h.update(repr(x).encode())
        h.update(b"|")
    return f"{call}-{h.hexdigest()[:24]}"


class RefResults:
    def __init__(self, name, lib_name):
        self.path = os.path.join(ROOT, "tests", "golden", f"ref_{name}_results.npz")
        self.lib_path = os.path.join(ROOT, "oracle", "_ref", lib_name)
        self._lib, self._stored, self._new = None, None, {}
        if RECORD:
            atexit.register(self._save)

    def get(self, call, inputs, live):
        key = _key(call, inputs)
        if RECORD:
            if self._lib is None:
                self._lib = C.CDLL(self.lib_path)
            out = tuple(live(self._lib))
            self._new[key] = out
            return out
        if self._stored is None:
            self._stored = np.load(self.path)
        n = int(self._stored[key + ".n"])          # KeyError: inputs no recorded call had -- record the fixtures again
        return tuple(self._stored[f"{key}.{i}"][()] for i in range(n))

    def _save(self):
        flat = {}
        for key, out in self._new.items():
            flat[key + ".n"] = np.array(len(out))
            for i, v in enumerate(out):
                flat[f"{key}.{i}"] = np.asarray(v)
        np.savez_compressed(self.path, **flat)
