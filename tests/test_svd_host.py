"""The host steps of the truncated SVD (smallk_amd/csrc/svd_host.h: cyclic Jacobi eigendecomposition of the l x l Gram matrix
and the orthonormalising matrix M = E Lambda^(-1/2)) under AddressSanitizer + UndefinedBehaviorSanitizer, as a stand-alone
program (tests/svd_host/jacobi_check.cpp) that includes the header by itself.  The program makes the checks and prints one line
per matrix: l = 1, l = 128, the zero matrix, repeated eigenvalues, a Gram matrix of exact rank 3 at l = 20, eigenvalues
2^-60 .. 1."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENV = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0:halt_on_error=1", UBSAN_OPTIONS="print_stacktrace=1:halt_on_error=1")


def test_jacobi_and_orth_matrix_are_clean_and_within_their_bars(tmp_path):
    exe = tmp_path / "jacobi_check"
    b = subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-fno-omit-frame-pointer", "-fsanitize=address,undefined",
                        os.path.join(ROOT, "tests", "svd_host", "jacobi_check.cpp"), "-o", str(exe)], capture_output=True, text=True)
    assert b.returncode == 0, b.stderr[-3000:]
    r = subprocess.run([str(exe)], capture_output=True, text=True, timeout=300, env=ENV)
    text = r.stdout + r.stderr
    print(text)
    assert "AddressSanitizer" not in text and "runtime error:" not in text and "LeakSanitizer" not in text, text[-4000:]
    assert r.returncode == 0, text[-3000:]
    assert "jacobi_check: all ok" in r.stdout
    assert r.stdout.count("zero_cols=1 ok\n") == 7 and "FAILED" not in r.stdout
