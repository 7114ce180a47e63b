"""The one-root hit acceptance of the accelerated walks
(a_dive_into_ray_tracing_amd/csrc/rtmi_accept.h, the code resolve_root and
resolve_key run on the device) against the literal two-root rule, on the CPU:
tests/native/resolve_accept.cpp includes the header, is built with g++ and
run over 1e7 random (hb, disc >= 0, a, t_max, later) tuples with a fixed
seed, each also with t_max forced to r1, to r2 and to +inf, and over the
product of the special values (+-0, 0.001f and its two neighbours,
denormals, +-inf, NaN, 3.4e38).  No difference in the decision or in the
accepted root's bits is allowed, at least 1e6 exact ties must have been
exercised, and the tie callback (the scene-order compare, which the kernels
keep off the common path) must be called for exact ties only."""
import json
import os
import shutil
import subprocess

import pytest

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(REPO, "tests", "native", "resolve_accept.cpp")
N_RANDOM = 10_000_000


@pytest.fixture(scope="module")
def result(tmp_path_factory):
    cxx = shutil.which("g++")
    assert cxx, "g++ is needed to build tests/native/resolve_accept.cpp"
    exe = str(tmp_path_factory.mktemp("resolve_accept") / "resolve_accept")
    subprocess.run([cxx, "-O2", "-std=c++17", "-ffp-contract=off", "-Wall", "-Werror", "-o", exe, SRC], check=True)
    p = subprocess.run([exe, str(N_RANDOM)], capture_output=True, text=True)
    assert p.returncode in (0, 1), p.stderr
    return p.returncode, json.loads(p.stdout.strip().splitlines()[-1]), p.stderr


def test_one_root_form_equals_two_root_rule(result):
    rc, d, err = result
    assert d["differences"] == 0 and rc == 0, (d, err)


def test_inputs_exercise_ties_and_acceptances(result):
    """Conditions on the inputs: the forcing of t_max makes the exact ties, and
    a good part of the cases accept a root."""
    _, d, _ = result
    assert d["cases"] >= 4 * N_RANDOM, d
    assert d["ties"] >= 1_000_000, d
    assert d["accepted"] >= 1_000_000, d


def test_scene_order_is_asked_for_exact_ties_only(result):
    _, d, _ = result
    assert d["later_calls_off_tie"] == 0, d
