"""The move-only owners of the engines' device resources (csrc/pbre_devmem.hpp), host only: a stand-alone program compiles the header
against counting stand-ins of hipMalloc / hipFree / the event and stream calls and checks construction, move, release on an early
return out of a set-up function, and double release; then grow, upload_once and Stage of csrc/pbre_devwork.hpp (the buffers of the
units that read the state, and the slice layout of their host-buffer variants) -- under AddressSanitizer and UBSan, so a leak or a
double free fails the run."""
import os
import shutil
import subprocess

import pytest

HERE = os.path.dirname(os.path.abspath(__file__))


def test_owners_release_exactly_what_was_made(tmp_path):
    cxx = shutil.which("g++")
    if cxx is None:
        pytest.fail("no g++")
    exe = str(tmp_path / "devmem_test")
    # (the sanitizer runtimes linked into the program itself: it runs wherever the suite does)
    subprocess.check_call([cxx, "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-static-libasan",
                           "-static-libubsan", "-o", exe, os.path.join(HERE, "host_emu", "devmem_test.cpp")])
    r = subprocess.run([exe], capture_output=True, text=True, env=dict(os.environ, ASAN_OPTIONS="detect_leaks=1"))
    assert r.returncode == 0, r.stdout + r.stderr
    assert "devmem_test OK" in r.stdout
