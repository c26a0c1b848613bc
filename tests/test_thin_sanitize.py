"""The host bookkeeping of sgtd_thin_clouds under AddressSanitizer + UndefinedBehaviorSanitizer on the CPU: the engine
compiled for the host only and linked against tests/cpp/sanitize/hip_stub.cpp and tests/cpp/sanitize/thin_driver.cpp, a
stand-alone program, the way test_stored_voxel_sanitize.py builds its driver.  The driver's launch hook does on the host
what the call's kernels would if every finite point were a cell of its own, so the call sizes, fills and hands out its
output: the getters before a run, the argument errors and caps with the earlier results kept, empty batches and clouds,
both strides, a shrinking then a growing size on one handle, a batch with every point dropped (K = 0), 256 clouds, a
view, the timed form."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SAN = os.path.join(ROOT, "tests", "cpp", "sanitize")
ASAN = ["-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-fno-omit-frame-pointer"]
ENV = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0", UBSAN_OPTIONS="print_stacktrace=1")
HIPCC = "/opt/rocm/bin/hipcc"
CLANG = "/opt/rocm/lib/llvm/bin/clang++"


@pytest.mark.skipif(not (os.path.exists(HIPCC) and os.path.exists(CLANG)), reason="needs the ROCm compilers (host-only compile of the engine)")
def test_thin_host_code_under_asan_and_ubsan(tmp_path):
    hip = [HIPCC, "-O1", "-g", "-std=c++17", "--offload-arch=gfx950", "-ffp-contract=off", "--cuda-host-only", "-Wno-unused-function",
           "-Wno-unused-result"] + ASAN
    objs = {n: str(tmp_path / (n + ".o")) for n in ("accel", "driver", "stub", "fatbin")}
    subprocess.check_call(hip + ["-c", os.path.join(ROOT, "sgtd_amd", "csrc", "sgtd_accel.hip"), "-o", objs["accel"]], stderr=subprocess.DEVNULL)
    subprocess.check_call(hip + ["-c", "-x", "hip", os.path.join(SAN, "thin_driver.cpp"), "-o", objs["driver"]], stderr=subprocess.DEVNULL)
    subprocess.check_call([CLANG, "-O1", "-g", "-std=c++17", "-D__HIP_PLATFORM_AMD__", "-I/opt/rocm/include"] + ASAN +
                          ["-c", os.path.join(SAN, "hip_stub.cpp"), "-o", objs["stub"]], stderr=subprocess.DEVNULL)
    # the host objects refer to their (absent) device code objects by a symbol whose name carries a hash of the translation unit
    undefined = subprocess.run(["nm", "-u", objs["accel"], objs["driver"]], capture_output=True, text=True, check=True).stdout
    names = sorted({w for line in undefined.splitlines() for w in line.split() if w.startswith("__hip_fatbin_")})
    assert names
    src = tmp_path / "fatbin.cpp"
    src.write_text("".join('extern "C" const char %s[16] = {0};\n' % n for n in names))
    subprocess.check_call([CLANG, "-c", str(src), "-o", objs["fatbin"]])
    exe = str(tmp_path / "thin_asan")
    subprocess.check_call([CLANG] + ASAN + [objs["accel"], objs["driver"], objs["stub"], objs["fatbin"], "-pthread", "-o", exe])
    out = subprocess.run([exe], capture_output=True, text=True, timeout=600, env=ENV)
    assert out.returncode == 0, out.stdout[-3000:] + out.stderr[-6000:]
    assert "thin_clouds under the sanitizers: ok" in out.stdout and "ERROR: " not in out.stderr, out.stdout[-2000:] + out.stderr[-4000:]
