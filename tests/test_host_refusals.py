"""The exits of the library's host code that give up a plan, an event or a timer, under AddressSanitizer + UBSan in a process of
their own: tests/host_refusals.c -- plain C against include/cloudy_hip.h -- is compiled with the sanitizers, linked against the
host sanitizer build of the library (`make -C cloudy.jl_amd/csrc asan`, as tests/test_host_sanitizers.py) and run as an ordinary
child.  The executable is linked against the sanitizer runtime, so nothing is preloaded.  CPU only: with a device present
cloudy_plan_create succeeds and the exit that frees a completely built host plan (CLOUDY_ENODEVICE) is not taken."""
import os
import re
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIBDIR = os.path.join(ROOT, "cloudy.jl_amd")
CLANG = "/opt/rocm/lib/llvm/bin/clang"
OURS = re.compile(r"cloudy_hip\.hip|host_\w+\.hpp")


def _build(tmp_path):
    r = subprocess.run(["make", "-C", os.path.join(LIBDIR, "csrc"), "-j", "8", "asan"], capture_output=True, text=True)
    if r.returncode != 0 or not os.path.exists(os.path.join(LIBDIR, "libcloudy_hip_asan.so")):
        pytest.skip("host sanitizer build not available: " + (r.stderr or r.stdout)[-300:])
    rt = subprocess.run([CLANG, "-print-file-name=libclang_rt.asan-x86_64.so"], capture_output=True, text=True).stdout.strip()
    if not os.path.isfile(rt):
        pytest.skip("clang's ASan runtime not found")
    exe = str(tmp_path / "host_refusals")
    cmd = [CLANG, "-O1", "-g", "-Wall", "-Werror", "-fsanitize=address,undefined", "-shared-libsan", "-fno-omit-frame-pointer",
           "-I" + os.path.join(ROOT, "include"), os.path.join(ROOT, "tests", "host_refusals.c"), "-o", exe, "-L" + LIBDIR,
           "-l:libcloudy_hip_asan.so", "-Wl,-rpath," + LIBDIR, "-Wl,-rpath,/opt/rocm/lib", "-Wl,-rpath," + os.path.dirname(rt), "-lm"]
    r = subprocess.run(cmd, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    return exe


def _run(exe, detect_leaks):
    env = {k: v for k, v in os.environ.items() if k not in ("LD_PRELOAD", "CLOUDY_HIP_LIB")}
    # (a leak ends the run with the program's own status: the reports are judged below, frame by frame)
    env.update(ASAN_OPTIONS=f"detect_leaks={detect_leaks}:abort_on_error=0", LSAN_OPTIONS="exitcode=0",
               UBSAN_OPTIONS="halt_on_error=1:print_stacktrace=1", ASAN_SYMBOLIZER_PATH=os.path.join(os.path.dirname(CLANG), "llvm-symbolizer"),
               CLOUDY_HIP_CACHE_DIR="")
    return subprocess.run([exe], env=env, capture_output=True, text=True, timeout=300)


def test_every_host_refusal_frees_what_it_built_under_asan_ubsan(tmp_path, cloudy):
    """Every descriptor refusal through cloudy_plan_create and cloudy_jit_selfcheck, the CLOUDY_ENODEVICE exit of served
    descriptors, the timers and cloudy_time_coal_rhs with arguments and events that fail: exit status 0, no AddressSanitizer or
    UBSan report, and no leak report with a frame in cloudy_hip.hip or a host_*.hpp (the HIP runtime's own allocations, which a
    process without a device may keep, are not the library's).  Where LeakSanitizer cannot start (it says so) the run is repeated
    without leak detection."""
    if cloudy.device_count() > 0:
        pytest.skip("GPU present: the exits without a device are not taken")
    exe = _build(tmp_path)
    p = _run(exe, 1)
    if "LeakSanitizer has encountered a fatal error" in p.stderr or "LeakSanitizer does not work" in p.stderr:
        print("LeakSanitizer cannot start here: run without leak detection")
        p = _run(exe, 0)
    out = p.stdout + p.stderr
    assert p.returncode == 0, out[-4000:]
    assert "host_refusals ok" in p.stdout
    assert "runtime error" not in out and "ERROR: AddressSanitizer" not in out, out[-4000:]
    leaks = [b for b in out.split("\n\n") if re.search(r"\bleak of \d+ byte", b)]
    ours = [b for b in leaks if OURS.search(b)]
    print(f"leak reports: {len(leaks)}, with a frame of the library's host code: {len(ours)}")
    assert not ours, "\n\n".join(ours)[-4000:]
