"""The host side every constrained schedule call shares, without a GPU: csrc/ksched_full.h's check-and-pack under each of
the seven calls' kinds (the table of csrc/ksched_exact.h), as a stand-alone program -- every refusal with its code and
text, the order where two apply, and what is packed against the constraints' own packers -- plain and under the host
sanitizers; and the programs of the single checkers, which must still build warning-free beside it."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def build_check(tmp_path, source, name, extra):
    cxx = shutil.which("g++") or shutil.which("c++")
    assert cxx, "a C++ compiler"
    exe = str(tmp_path / name)
    subprocess.run([cxx, "-std=c++17", "-O1", "-Wall", "-Werror", *extra, "-I" + os.path.join(ROOT, "include"),
                    "-I" + os.path.join(ROOT, "k8s-scheduler_amd", "csrc"),
                    os.path.join(ROOT, "tests", "diag", source), "-o", exe], check=True)
    return exe


def test_check_program_builds_and_passes(tmp_path):
    exe = build_check(tmp_path, "kind_check_main.cpp", "kind_check", [])
    out = subprocess.run([exe], check=True, capture_output=True, text=True).stdout
    assert "all checks passed" in out


def test_check_program_passes_under_the_host_sanitizers(tmp_path):
    """The same program, its own executable, built with the address and undefined-behaviour sanitizers and run directly:
    every array is allocated at exactly the length its case states, so a read beyond what the arguments allow is a
    report (and a failed run)."""
    exe = build_check(tmp_path, "kind_check_main.cpp", "kind_check_san",
                      ["-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"])
    out = subprocess.run([exe], check=True, capture_output=True, text=True).stdout
    assert "all checks passed" in out


@pytest.mark.parametrize("source", ["full_check_main.cpp", "affinity_check_main.cpp", "gang_check_main.cpp"])
def test_the_other_check_programs_still_build_and_pass(source, tmp_path):
    """(why_check_main and dryrun_check_main are built and run by test_why_host and test_dryrun_host.)"""
    exe = build_check(tmp_path, source, source[:-4], [])
    out = subprocess.run([exe], check=True, capture_output=True, text=True).stdout
    assert "every expectation met" in out
