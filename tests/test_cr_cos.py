"""cr_cos (epnet_amd/csrc/cr_cos.h): the float64 cosine of the AP evaluator's orientation similarity, evaluated in double-double
and rounded once. Built for the host from the same header the kernel includes, with contraction off as in the library's build.

Yardstick: the C library's cos (math.cos), which is correctly rounded for all but about one argument in a thousand and never
more than one ulp off; and four arguments on which it is NOT, with the correctly rounded results (from 200-bit arithmetic)
written out."""
import math
import os
import shutil
import struct
import subprocess

import numpy as np
import pytest

from conftest import ROOT

# argument -> correctly rounded cos; the C library returns the neighbouring float64 on each of them
HARD = {
    4.567349496856238: -0.14453149878247587,
    18.385295921510021: 0.89415315370830373,
    42567.30212606123: 0.28831461851322621,
    -1.433785104085775: 0.13658296071365619,
}


@pytest.fixture(scope="module")
def cr_cos(tmp_path_factory):
    cxx = shutil.which("g++") or shutil.which("c++") or shutil.which("clang++")
    assert cxx, "a host C++ compiler is needed"
    exe = str(tmp_path_factory.mktemp("cr_cos") / "cr_cos_selftest")
    subprocess.check_call([cxx, "-O2", "-std=c++17", "-ffp-contract=off", "-I", os.path.join(ROOT, "epnet_amd", "csrc"),
                           os.path.join(ROOT, "tests", "cr_cos_selftest.cpp"), "-o", exe])

    def run(values):
        out = subprocess.run([exe] + [repr(float(v)) for v in values], capture_output=True, text=True, check=True, timeout=60)
        return [struct.unpack("<d", struct.pack("<Q", int(line, 16)))[0] for line in out.stdout.split()]
    return run


def test_hard_cases_and_special_values(cr_cos):
    args = list(HARD)
    assert cr_cos(args) == [HARD[a] for a in args]
    assert any(math.cos(a) != HARD[a] for a in args), "these are arguments the C library rounds the other way"
    assert cr_cos([0.0, -0.0]) == [1.0, 1.0]
    assert all(math.isnan(v) for v in cr_cos([float("nan"), float("inf")]))
    assert cr_cos([1e300, -3e7]) == [math.cos(1e300), math.cos(-3e7)]   # beyond the reduction's exact range: the library's


def test_against_the_c_library(cr_cos):
    rng = np.random.default_rng(3)
    quarter = [k * math.pi / 4 for k in range(-26, 27)]   # the reduction's and the quadrants' boundaries, |alpha difference| <= 20
    args = quarter + [math.nextafter(q, 0.0) for q in quarter] + rng.uniform(-20.0, 20.0, 3000).tolist() + rng.uniform(-1e5, 1e5, 500).tolist()
    got, differ = cr_cos(args), 0
    for a, g in zip(args, got):
        w = math.cos(a)
        if g != w:
            differ += 1
            assert g in (math.nextafter(w, -2.0), math.nextafter(w, 2.0)), (a, g, w)
    print("%d of %d arguments differ from the C library's cos, each by one ulp" % (differ, len(args)))
    assert differ <= len(args) // 100
