"""The exact division by a known divisor (csrc/hrt_div.h) against `/`, bit for bit, without a GPU (tests/div/div_check.cpp).

div_check is built with g++ -mfma -ffp-contract=off and the address and undefined-behaviour sanitizers (make div_check) and is an
ordinary executable.  What it covers is fixed here, not by what the code under test gives:
  known divisors  every |R| and |U| of the five configuration scenes and the nine demo scenes (through the host layer), 6, 1920,
                  1080, 3840, 2160, all-ones significands (which the theorem behind the sequence leaves out) up to both ends of
                  the window, nextafter(1, +-inf), random and negative divisors: >= 64 of them x all 2^24 numerators of [1, 4)
  guard edges     2^-61, 2^-60, 2^60, 2^61 and their neighbours, denormals, +-0, +-inf, NaN as numerator and as divisor
  normalise       normalize_shared on >= 10^7 vectors: cube samples, normalised vectors, a +-0 component, arbitrary bit patterns
Every comparison is on the bits (NaN against NaN)."""
import json
import os
import subprocess

import pytest

from conftest import PKG, ROOT


@pytest.fixture(scope="module")
def report():
    subprocess.run(["make", "-s", "-C", PKG, "libhrt_host.so", "div_check"], check=True)
    r = subprocess.run([os.path.join(PKG, "div_check"), os.path.join(ROOT, "assets")], capture_output=True, text=True)
    assert r.stderr == "", r.stderr[-4000:]
    out = json.loads(r.stdout)
    out["rc"] = r.returncode
    return out


def test_known_divisors_equal_the_division_for_every_numerator(report):
    k = report["known"]
    assert k["divisors"] >= 64 and k["scene_divisors"] >= 8 and k["numerators"] == 1 << 24
    assert k["mismatches"] == 0


def test_guard_edges_equal_the_division(report):
    e = report["edges"]
    assert e["pairs"] == 15 * 15 * 4 and 0 < e["fast"] < e["pairs"]  # both sides of the guard are reached
    assert e["mismatches"] == 0


def test_two_quotients_under_one_guard_equal_the_divisions(report):
    p = report["pairs"]
    assert p["pairs"] >= 2_000_000 and 0 < p["fast"] < p["pairs"]
    assert p["mismatches"] == 0


def test_normalize_shared_equals_the_three_divisions(report):
    n = report["normalize"]
    assert n["vectors"] >= 10_000_000 and n["fast"] > n["vectors"] // 2  # (a zero component is left to `/`: a quarter of the vectors)
    assert n["mismatches"] == 0 and report["rc"] == 0


def test_the_header_is_plain_cxx():
    with open(os.path.join(PKG, "csrc", "hrt_div.h")) as f:
        src = f.read()
    assert "#include" not in src and "float4" not in src and "hip/" not in src
