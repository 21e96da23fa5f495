"""The drop-in claim of the boundary (north_star "drops into test.cpp unchanged"): the reference's own
caller, test.cpp, compiles against include/line2Dup.h and links against the facade library, unchanged.
build() makes that binary by oracle/ref_caller.mk (the source is read from the reference tree and piped to the
compiler; nothing of it is copied) into oracle/_ref/, which is kept out of git; this test checks what it made."""
import os
import subprocess

from conftest import ROOT

EXE = os.path.join(ROOT, "oracle", "_ref", "ref_test_cpp")


def test_reference_test_cpp_compiles_and_links_against_the_facade():
    assert os.path.exists(EXE), "oracle/_ref/ref_test_cpp missing: run __graft_entry__.build() where the reference tree is present"
    log = open(EXE + ".log").read()
    assert "error" not in log, log[-3000:]
    r = subprocess.run(["ldd", EXE], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    assert "not found" not in r.stdout, r.stdout
    libs = {line.split()[0]: line for line in r.stdout.splitlines() if "=>" in line}
    for name in ("libsbm_facade.so", "libsbm_hip.so"):
        assert name in libs, r.stdout
        assert os.path.realpath(libs[name].split("=>")[1].split()[0]) == os.path.realpath(
            os.path.join(ROOT, "shape_based_matching_amd", name)), libs[name]
