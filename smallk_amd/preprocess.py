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
from smallk_amd.solver import SparseMatrix, initialize, is_initialized, load_matrix_market, _is_tensor, _stream_of, _tensor_view

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

    def vocabulary(self) -> "Vocabulary":
        """What the fit leaves for documents that arrive later: its surviving terms, their idf and its boolean_mode, on the
        device.  Only a fit has one: an applied result raises SmallkError(FAILURE)."""
        h = C.c_void_p()
        L.check(L.lib().smk_preprocess_result_vocabulary(self._h, C.byref(h)), "smk_preprocess_result_vocabulary")
        return Vocabulary._from_handle(h)

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


class Vocabulary:
    """A fitted term set on the device: ``term_indices`` (the surviving terms' original indices, ascending), ``idf`` (fp64, as
    the fit computed it), ``height_in`` (the term count of the fit's input) and the fit's ``boolean_mode``.  ``apply`` turns raw
    term counts of new documents, in the original term numbering, into the tf-idf matrix of the fit's term space."""

    def __init__(self, term_indices, idf, height_in, boolean_mode=0):
        if not is_initialized():
            initialize(-1)
        term = _u32(term_indices)
        w = np.ascontiguousarray(idf, dtype=np.float64)
        if term.ndim != 1 or w.shape != term.shape:
            raise ValueError("Vocabulary: term_indices and idf are 1-D arrays of one length")
        self._h = C.c_void_p()
        L.check(L.lib().smk_vocabulary_create(int(height_in), int(term.size), term.ctypes.data_as(_up),
                                              w.ctypes.data_as(C.POINTER(C.c_double)), int(boolean_mode), C.byref(self._h)),
                "smk_vocabulary_create")
        self._read_sizes()

    @classmethod
    def _from_handle(cls, handle):
        self = cls.__new__(cls)
        self._h = handle
        self._read_sizes()
        return self

    def _read_sizes(self):
        hi, h, b = C.c_uint(), C.c_uint(), C.c_int()
        L.check(L.lib().smk_vocabulary_sizes(self._h, C.byref(hi), C.byref(h), C.byref(b)), "smk_vocabulary_sizes")
        self.height_in, self.height, self.boolean_mode = hi.value, h.value, b.value

    def _download(self):
        term = np.zeros(self.height, dtype=np.uint32)
        idf = np.zeros(self.height, dtype=np.float64)
        L.check(L.lib().smk_vocabulary_download(self._h, term.ctypes.data_as(_up), idf.ctypes.data_as(C.POINTER(C.c_double))),
                "smk_vocabulary_download")
        return term, idf

    @property
    def term_indices(self):
        return self._download()[0]

    @property
    def idf(self):
        return self._download()[1]

    def save(self, path):
        """The vocabulary as an .npz file (term_indices, idf, height_in, boolean_mode) for a later process."""
        term, idf = self._download()
        with open(path, "wb") as f:
            np.savez(f, term_indices=term, idf=idf, height_in=np.uint32(self.height_in), boolean_mode=np.int32(self.boolean_mode))

    @classmethod
    def load(cls, path):
        with np.load(path) as z:
            return cls(z["term_indices"], z["idf"], int(z["height_in"]), int(z["boolean_mode"]))

    def apply(self, col_offsets, row_indices=None, data=None, width=None, *, min_terms=0, boolean_mode=-1) -> PreprocessResult:
        """Score new documents.  The input is a CSC term-count matrix with ``height_in`` rows: host arrays ``(col_offsets,
        row_indices, data, width)``, one scipy CSC matrix, or torch CSC tensors in GPU memory (1-D ``ccol_indices``,
        ``row_indices``, ``values``, or one ``torch.sparse_csc_tensor``), which never leave the device.  ``min_terms`` drops a
        document with fewer surviving entries (0 keeps all, empty ones included); ``boolean_mode`` -1 is the fit's.  The
        result's ``ok`` is False when every document was dropped."""
        o = L.ApplyOptions(int(min_terms), int(boolean_mode))
        h = C.c_void_p()
        first = col_offsets
        if _is_tensor(first):
            import torch
            if first.layout == torch.sparse_csc:
                if first.dim() != 2 or first.shape[0] != self.height_in:
                    raise ValueError(f"Vocabulary.apply: expected a sparse tensor with {self.height_in} rows, got shape {tuple(first.shape)}")
                col_offsets, row_indices, data, width = first.ccol_indices(), first.row_indices(), first.values(), first.shape[1]
            if row_indices is None or data is None:
                raise TypeError("Vocabulary.apply: ccol_indices, row_indices and values, or one sparse CSC tensor")
            width = int(col_offsets.numel() - 1 if width is None else width)
            if col_offsets.numel() != width + 1 or row_indices.numel() != data.numel():
                raise ValueError("Vocabulary.apply: ccol_indices needs width + 1 entries, row_indices as many as values")
            nnz = int(data.numel())
            views = []
            for t, what, kinds in ((col_offsets, "ccol_indices", "index"), (row_indices, "row_indices", "index"), (data, "values", "factor")):
                if nnz == 0 and what != "ccol_indices":
                    views.append((t, C.c_void_p(), L.IDX_I32 if kinds == "index" else L.DT_F64))
                else:
                    t = t.contiguous()
                    views.append((t,) + _tensor_view(t, f"Vocabulary.apply({what})", ndim=1, kinds=kinds)[:2])
            (co, co_p, co_t), (ri, ri_p, ri_t), (va, va_p, va_t) = views
            rc = L.lib().smk_vocabulary_apply_device(self._h, C.byref(o), width, nnz, co_p, co_t, ri_p, ri_t, va_p, va_t,
                                                     _stream_of(co), C.byref(h))
            where = "smk_vocabulary_apply_device"
        else:
            if hasattr(first, "tocsc"):
                A = first.tocsc()
                if A.shape[0] != self.height_in:
                    raise ValueError(f"Vocabulary.apply: expected a matrix with {self.height_in} rows, got shape {A.shape}")
                col_offsets, row_indices, data, width = A.indptr, A.indices, A.data, A.shape[1]
            if row_indices is None or data is None:
                raise TypeError("Vocabulary.apply: col_offsets, row_indices, data and width, or one scipy sparse matrix")
            co, ri = _u32(col_offsets), _u32(row_indices)
            va = np.ascontiguousarray(data, dtype=np.float64)
            width = int(co.size - 1 if width is None else width)
            if co.size != width + 1:
                raise ValueError("Vocabulary.apply: col_offsets needs width + 1 entries")
            nnz = int(co[-1]) - int(co[0])
            if ri.size < int(co[-1]) or va.size < int(co[-1]):
                raise ValueError("Vocabulary.apply: row_indices and data are shorter than col_offsets says")
            rc = L.lib().smk_vocabulary_apply(self._h, C.byref(o), width, nnz, co.ctypes.data_as(_up), ri.ctypes.data_as(_up),
                                              va.ctypes.data_as(C.POINTER(C.c_double)), C.byref(h))
            where = "smk_vocabulary_apply"
        if rc not in (L.OK, L.FAILURE):
            L.check(rc, where)
        return PreprocessResult(h, rc)

    def close(self):
        if self._h:
            L.lib().smk_vocabulary_destroy(self._h)
            self._h = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


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

    def vocabulary(self) -> Vocabulary:
        """The fitted vocabulary of the last ``preprocess()``, for documents that arrive later (``Vocabulary.apply``)."""
        if self._res is None:
            raise RuntimeError("preprocess() has not produced a result")
        return self._res.vocabulary()

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
