"""The stand-alone host programs of csrc/ (vlr_*_host.cpp: a kernel's header compiled for the CPU, with a main of its own) built under
the sanitizers, for test_basepileup_host.py, test_indelpileup_host.py, test_fragpileup_host.py, test_fragrealign_host_program.py,
test_fragment_indel_host.py and test_ingest_host_program.py (whose program links the host units of the front door).  A plain helper
module: the `program` fixtures stay in those files."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "varlociraptor_amd", "csrc")
SAN = ["-fsanitize=address,undefined", "-fno-sanitize-recover=undefined"]


def build(tmp_path_factory, source_name, extra_sources=(), libs=()):
    """path of the program built from csrc/<source_name>.cpp (and the csrc/ files `extra_sources`, linked with `libs`) with
    -fsanitize=address,undefined; skips without a compiler that can"""
    cxx = shutil.which("c++") or shutil.which("g++") or shutil.which("clang++")
    if cxx is None:
        pytest.skip("no system C++ compiler")
    out = os.path.join(CSRC, "build", "host")
    try:
        os.makedirs(out, exist_ok=True)
        open(os.path.join(out, ".w"), "w").close()
    except OSError:
        out = str(tmp_path_factory.mktemp("host_build"))
    probe = os.path.join(out, "probe_%s" % source_name)   # (a name of its own: the modules may build at the same time)
    with open(probe + ".cpp", "w") as f:
        f.write("int main() { return 0; }\n")
    # the sanitizer runtimes linked statically where the compiler can (nothing preloaded into the process can then come before them)
    for static in (["-static-libasan", "-static-libubsan"], []):
        flags = SAN + static
        r = subprocess.run([cxx] + flags + [probe + ".cpp", "-o", probe], capture_output=True, text=True)
        if r.returncode == 0 and subprocess.run([probe], capture_output=True).returncode == 0:
            break
    else:
        pytest.skip("the system compiler has no usable -fsanitize=address,undefined: " + r.stderr[-200:])
    exe = os.path.join(out, source_name)
    subprocess.check_call([cxx, "-std=c++17", "-O1", "-g", "-Wall", "-Werror", "-ffp-contract=off"] + flags +
                          [os.path.join(CSRC, f) for f in (source_name + ".cpp",) + tuple(extra_sources)] + ["-o", exe] + list(libs))
    return exe
