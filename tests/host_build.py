"""Compiles a test's host program against the plan headers of csrc/ (no device code), with the system C++ compiler or hipcc."""
import os
import shutil
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "panic3d-anime-reconstruction_amd", "csrc")


def compile_host(tmp_path, source):
    """tests/<source> -> an executable under tmp_path; returns its path."""
    exe = str(tmp_path / os.path.splitext(source)[0])
    cxx = shutil.which(os.environ.get("CXX", "c++")) or shutil.which("g++")
    if cxx is None:
        import panic3d_amd
        cxx = panic3d_amd._build._hipcc()
    subprocess.check_call([cxx, "-std=c++17", "-O1", "-Wall", "-Werror", "-I", CSRC, os.path.join(ROOT, "tests", source), "-o", exe])
    return exe
