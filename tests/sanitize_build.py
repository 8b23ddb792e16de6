"""The one build of the stand-alone programs that drive the host layer of libvfgs_hip on the CPU (tests/sanitize*/*.cpp over
tests/sanitize/walks.h): the compile line, the objects every such program shares, how a program is run, and the two test bodies of a walk
program.  A plain helper module; tests/test_sanitize_*_cpu.py, tests/test_*_abi_cpu.py, tests/test_entry_matrix_cpu.py and
tests/test_seed_segments_cpu.py compile through it and through nothing else.

The three host sources and the model of the HIP runtime (tests/sanitize/hip_stub.cpp) are compiled to objects once per flavour -- ASan + UBSan,
TSan, none, and none at -O2 for the model libraries that two tests load and time -- and per Python process, into a directory of that process's
own that is removed when it ends, so test processes that run side by side share no file.  Every test links its own translation units against
those objects.  The programs have their own main and are run directly:
nothing is loaded into Python under a sanitizer and nothing is preloaded."""
import atexit
import functools
import os
import shutil
import subprocess
import tempfile
from pathlib import Path

import pytest

ROOT = Path(__file__).resolve().parent.parent
CSRC = ROOT / "versatilefilmgrain_amd" / "csrc"
SAN = ROOT / "tests" / "sanitize"
HOST_SOURCES = [CSRC / "vfgs_host.cpp", CSRC / "vfgs_fw_host.cpp", CSRC / "vfgs_cfg_host.cpp"]
STUB = SAN / "hip_stub.cpp"
HIP_INCLUDE = Path(os.environ.get("ROCM_PATH", "/opt/rocm")) / "include"

# a flavour: the optimisation level, then the sanitizer's flags
ASAN_UBSAN = ("-O1", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined")
TSAN = ("-O1", "-fsanitize=thread")
PLAIN = ("-O1",)
OPTIMISED = ("-O2",)      # the model libraries that two tests load into a child Python and time

HAVE_TOOLS = shutil.which("g++") is not None and (HIP_INCLUDE / "hip" / "hip_runtime_api.h").exists()
needs_gxx = pytest.mark.skipif(not HAVE_TOOLS, reason="needs g++ and the HIP headers")


def gxx(flavour, *args):
    """g++ with the flags every translation unit and every link of a flavour gets"""
    return subprocess.run(["g++", "-std=c++17", "-g", *flavour, "-fno-omit-frame-pointer", "-D__HIP_PLATFORM_AMD__", f"-I{HIP_INCLUDE}",
                           f'-DVFGS_FW_TABLES_PATH="{CSRC / "fw_tables.bin"}"', *map(str, args), "-pthread"], capture_output=True, text=True)


@functools.lru_cache(maxsize=None)
def _scratch():
    d = Path(tempfile.mkdtemp(prefix="vfgs_sanitize_"))
    atexit.register(shutil.rmtree, d, ignore_errors=True)
    return d


@functools.lru_cache(maxsize=None)
def obj(flavour, source, pic=False):
    """the object of one source in one flavour, compiled once per process"""
    source = Path(source)
    out = _scratch() / ("_".join([source.stem, *(f.lstrip("-").replace("=", "_").replace(",", "_") for f in flavour), *(["pic"] if pic else [])]) + ".o")
    r = gxx(flavour, *(["-fPIC"] if pic else []), "-c", source, "-o", out)
    assert r.returncode == 0, r.stderr[-4000:]
    return out


def try_build(tmp, name, flavour, sources, extra=(), stub=True, shared=False):
    """Links tmp/name from `sources` (the program's own translation units: sources or objects), `extra` (further sources of the host layer,
    compiled once per flavour) and the shared objects of the host layer; stub=False leaves the shared model of the HIP runtime out, for a
    program that brings its own.  Returns (path, the link's CompletedProcess)."""
    exe = Path(tmp) / name
    shared_sources = [*HOST_SOURCES, *extra, *([STUB] if stub else [])]
    r = gxx(flavour, *(["-shared", "-fPIC"] if shared else []), *[obj(flavour, s, shared) for s in shared_sources], *sources, "-o", exe)
    return exe, r


def build(tmp, name, flavour, sources, extra=(), stub=True, shared=False):
    exe, r = try_build(tmp, name, flavour, sources, extra, stub, shared)
    assert r.returncode == 0, r.stderr[-4000:]
    return exe


def no_aslr_prefix():
    """GCC's ThreadSanitizer has a fixed memory layout and stops at start-up ("unexpected memory mapping") where the kernel
    randomises mappings more widely than it expects; it does not re-run itself without randomisation, so the walk is started
    that way (a personality of that one process) wherever setarch may do so."""
    cmd = ["setarch", os.uname().machine, "-R"]
    if shutil.which("setarch") and subprocess.run(cmd + ["true"], capture_output=True).returncode == 0:
        return cmd
    return []


def run(exe, env_extra, *walks, prefix=()):
    env = dict(os.environ, **env_extra)
    for k in ("VFGS_HIP_FRAME_HEIGHT", "VFGS_HIP_LINE_LOOKAHEAD", "LD_PRELOAD"):
        env.pop(k, None)
    r = subprocess.run([*prefix, str(exe), *walks], capture_output=True, text=True, env=env, timeout=600)
    return r


def run_asan_ubsan(exe):
    r = run(exe, {"ASAN_OPTIONS": "detect_leaks=1:abort_on_error=0", "UBSAN_OPTIONS": "print_stacktrace=1"})
    assert r.returncode == 0 and "ERROR" not in r.stderr and "runtime error" not in r.stderr, (r.stdout[-2000:], r.stderr[-6000:])
    return r


def check_asan_ubsan(exe, nwalks):
    r = run_asan_ubsan(exe)
    assert r.stdout.count(" ok ") == nwalks and "FAILED" not in r.stdout, r.stdout


def check_tsan(exe, nwalks):
    r = run(exe, {"TSAN_OPTIONS": "halt_on_error=0:second_deadlock_stack=1"}, prefix=no_aslr_prefix())
    assert r.returncode == 0 and "ThreadSanitizer" not in r.stderr, (r.stdout[-2000:], r.stderr[-6000:])
    assert r.stdout.count(" ok ") == nwalks and "FAILED" not in r.stdout, r.stdout
