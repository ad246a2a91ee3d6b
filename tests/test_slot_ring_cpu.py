"""The ring of block slots that the pitch, spectrum and resampler banks share (csrc/slot_ring.hip.h): its plain C++ part built with
a host compiler and run as a stand-alone program (tests/cpp/test_slot_ring.cpp) -- no GPU, no library."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_slot_ring_geometry_and_push_loop(tmp_path):
    exe = str(tmp_path / "test_slot_ring")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-Wall", "-Wextra", "-Werror", "-o", exe,
                           os.path.join(ROOT, "tests", "cpp", "test_slot_ring.cpp")])
    r = subprocess.run([exe], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    assert r.stdout.split()[1] == "checks" and int(r.stdout.split()[0]) > 100000, r.stdout
