"""The balance step's launch form (csrc/launch_form.hpp: per-leg normals, batch, warm, table, placed -> kernel family and two or
three wavefronts) against the table written out in tests/cpp/launch_form_check.cpp: a host program that includes nothing but
that header.  No GPU."""
import os
import subprocess

from conftest import ROOT


def test_the_launch_form_agrees_with_the_table(tmp_path):
    exe = str(tmp_path / "launch_form_check")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-Wall", "-Werror", "-I" + os.path.join(ROOT, "include"),
                           "-I" + os.path.join(ROOT, "quadruped_locomotion_amd", "csrc"), "-o", exe,
                           os.path.join(ROOT, "tests", "cpp", "launch_form_check.cpp")])
    p = subprocess.run([exe], capture_output=True, text=True, timeout=30)
    assert p.returncode == 0, p.stdout
    assert p.stdout.strip().endswith("rows 40 bad 0"), p.stdout
