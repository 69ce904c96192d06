"""preprocess_tf on the MI355X: term-document pruning and tf-idf scores (preprocessor/src/preprocess.cpp:81-232), and
pysmallk's ``Preprocessor`` class (pysmallk/interface/smallk_lib.pyx:1643-1815) on top of it.

``preprocess(...)`` is the C ABI call (``smk_preprocess``, include/smallk_amd.h) and returns a ``PreprocessResult`` whose
arrays stay on the device until asked for; ``PreprocessResult.matrix()`` hands the reduced matrix to the clustering and
the solver as a resident ``SparseMatrix`` without a trip through the host.  No CPU fallback.
"""
from __future__ import annotations

import argparse
import ctypes as C

import numpy as np

from smallk_amd import _lib as L
from smallk_amd.solver import SparseMatrix, initialize, is_initialized, load_matrix_market

_up = C.POINTER(C.c_uint)


def _u32(a):
    return np.ascontiguousarray(a, dtype=np.uint32)


class PreprocessResult:
    """Handle of one smk_preprocess result (device arrays)."""

    def __init__(self, handle, rc):
        self._h = handle
        self.ok = rc == L.OK
        h, w, n, it = C.c_uint(), C.c_uint(), C.c_uint(), C.c_uint()
        L.check(L.lib().smk_preprocess_result_sizes(self._h, C.byref(h), C.byref(w), C.byref(n), C.byref(it)),
                "smk_preprocess_result_sizes")
        self.height, self.width, self.nnz, self.iterations = h.value, w.value, n.value, it.value
        log = np.zeros(3 * self.iterations, dtype=np.uint32)
        if self.iterations:
            L.check(L.lib().smk_preprocess_result_log(self._h, log.ctypes.data_as(_up)), "smk_preprocess_result_log")
        self.log = [tuple(int(v) for v in log[3 * i:3 * i + 3]) for i in range(self.iterations)]
        up, dev = C.c_double(), C.c_double()
        L.lib().smk_preprocess_result_timing(self._h, C.byref(up), C.byref(dev))
        self.upload_ms, self.device_ms = up.value, dev.value

    def log_lines(self):
        """The reference's per-iteration lines ("\\t[i] height: h, width: w, nonzeros: n")."""
        return [f"\t[{i + 1}] height: {h}, width: {w}, nonzeros: {n}" for i, (h, w, n) in enumerate(self.log)]

    def download(self):
        """(term_indices, doc_indices, col_offsets, row_indices, scores) as numpy arrays."""
        if not self.ok:
            raise RuntimeError("preprocess failed: every column was pruned")
        term = np.zeros(self.height, dtype=np.uint32)
        doc = np.zeros(self.width, dtype=np.uint32)
        cp = np.zeros(self.width + 1, dtype=np.uint32)
        rows = np.zeros(self.nnz, dtype=np.uint32)
        scores = np.zeros(self.nnz, dtype=np.float64)
        L.check(L.lib().smk_preprocess_result_download(self._h, term.ctypes.data_as(_up), doc.ctypes.data_as(_up),
                                                       cp.ctypes.data_as(_up), rows.ctypes.data_as(_up),
                                                       scores.ctypes.data_as(C.POINTER(C.c_double))),
                "smk_preprocess_result_download")
        return term, doc, cp, rows, scores

    def matrix(self) -> SparseMatrix:
        """The reduced tf-idf matrix as a resident SparseMatrix (built on the device)."""
        h = C.c_void_p()
        L.check(L.lib().smk_preprocess_result_matrix(self._h, C.byref(h)), "smk_preprocess_result_matrix")
        m = SparseMatrix.__new__(SparseMatrix)
        m.height, m.ncols, m.width_global, m.col0 = self.height, self.width, self.width, 0
        m.storage, m.nnz, m._h = L.STORE_F32, self.nnz, h
        return m

    def write_mtx(self, path, precision=4):
        L.check(L.lib().smk_preprocess_write_mtx(self._h, str(path).encode(), int(precision)), "smk_preprocess_write_mtx")

    def close(self):
        if self._h:
            L.lib().smk_preprocess_result_destroy(self._h)
            self._h = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


def preprocess(height, width, col_offsets, row_indices, data, *, max_iter=1000, docs_per_term=3, terms_per_doc=5,
               boolean_mode=0) -> PreprocessResult:
    """smk_preprocess on a CSC term-count matrix.  The result's ``ok`` is False when every column was pruned (its ``log``
    still holds the iterations before that)."""
    if not is_initialized():
        initialize(-1)
    co, ri = _u32(col_offsets), _u32(row_indices)
    va = np.ascontiguousarray(data, dtype=np.float64)
    nnz = int(co[-1]) - int(co[0])
    o = L.PreprocessOptions(int(max_iter), int(docs_per_term), int(terms_per_doc), int(boolean_mode))
    h = C.c_void_p()
    rc = L.lib().smk_preprocess(C.byref(o), int(height), int(width), nnz, co.ctypes.data_as(_up), ri.ctypes.data_as(_up),
                                va.ctypes.data_as(C.POINTER(C.c_double)), C.byref(h))
    if rc not in (L.OK, L.FAILURE):
        L.check(rc, "smk_preprocess")
    return PreprocessResult(h, rc)


def _write_strings(path, strings, indices, n):
    with open(path, "w") as f:
        f.write("".join(f"{strings[i]}\n" for i in indices[:n]))


class Preprocessor:
    """pysmallk's ``Preprocessor`` (smallk_lib.pyx:1643-1815): same methods, keyword arguments and defaults.  Extra:
    ``reduced_matrix()``, the result as a resident ``SparseMatrix`` for ``hier_nmf2`` / ``NmfSolver``."""

    def __init__(self):
        self.height = self.width = 0
        self.dictionary, self.documents = [], []
        self._csc = None
        self._res = None
        self.scores, self.row_indices, self.col_offsets, self.term_ind, self.doc_ind = [], [], [], [], []

    def parser(self):
        parser = argparse.ArgumentParser()
        parser.add_argument("--indir", action="store", required=True, metavar="indir")
        parser.add_argument("--outdir", action="store", required=False, metavar="outdir", default="./")
        parser.add_argument("--docs_per_term", action="store", required=False, metavar="docs_per_term", default=3)
        parser.add_argument("--terms_per_doc", action="store", required=False, metavar="terms_per_doc", default=5)
        parser.add_argument("--maxiter", action="store", required=False, metavar="maxiter", default=1000)
        parser.add_argument("--precision", action="store", required=False, metavar="precision", default=4)
        parser.add_argument("--boolean_mode", action="store", required=False, metavar="boolean_mode", default=0)
        return parser.parse_args()

    def load_matrix(self, filepath="", height=0, width=0, nz=0, buffer=[], row_indices=[], col_offsets=[],
                    sparse_matrix=None):
        if filepath != "":
            data, indices, indptr, (h, w) = load_matrix_market(filepath)
            self._csc = (indptr, indices, data)
            self.height, self.width = h, w
        elif len(row_indices) > 0:
            co = _u32(col_offsets)
            self._csc = (co, _u32(row_indices), np.ascontiguousarray(buffer, dtype=np.float64))
            self.height, self.width = int(height), int(width)

    def load_dictionary(self, filepath="", dictionary=[]):
        if filepath != "":
            with open(filepath) as f:
                self.dictionary = f.read().split("\n")
        else:
            self.dictionary = dictionary

    def load_documents(self, filepath="", documents=[]):
        if filepath != "":
            with open(filepath) as f:
                self.documents = f.read().split("\n")
        else:
            self.documents = documents

    def preprocess(self, maxiter=1000, docsperterm=3, termsperdoc=5, boolean_mode=0):
        if self._res is not None:
            self._res.close()
            self._res = None
        co, ri, va = self._csc
        res = preprocess(self.height, self.width, co, ri, va, max_iter=maxiter, docs_per_term=docsperterm,
                         terms_per_doc=termsperdoc, boolean_mode=boolean_mode)
        if not res.ok:
            res.close()
            print("ERROR: preprocess()")
            return None
        self._res = res
        self.height, self.width = res.height, res.width
        term, doc, cp, rows, scores = res.download()
        self.term_ind, self.doc_ind = term.tolist(), doc.tolist()
        self.col_offsets, self.row_indices, self.scores = cp.tolist(), rows.tolist(), scores.tolist()

    def reduced_matrix(self) -> SparseMatrix:
        if self._res is None:
            raise RuntimeError("preprocess() has not produced a result")
        return self._res.matrix()

    def write_output(self, matrix_filepath, dict_filepath, docs_filepath, precision=4):
        self._res.write_mtx(matrix_filepath, precision)
        _write_strings(dict_filepath, self.dictionary, self.term_ind, self.height)
        _write_strings(docs_filepath, self.documents, self.doc_ind, self.width)

    def get_reduced_documents(self):
        return [self.documents[i] for i in self.doc_ind]

    def get_reduced_dictionary(self):
        return [self.dictionary[i] for i in self.term_ind]

    def get_reduced_scores(self):
        return self.scores

    def get_reduced_row_indices(self):
        return self.row_indices

    def get_reduced_col_offsets(self):
        return self.col_offsets

    def get_reduced_field(self, filepath="", values=[]):
        if filepath != "":
            with open(filepath) as f:
                values = f.read().split("\n")
        return [values[i] for i in self.doc_ind]
