"""The rules of hs_block and of the unit table (csrc/hs_blocks.h) on the CPU: tests/blocks_selftest.hip, a stand-alone program whose
allocation calls are counting stand-ins, is compiled with the library's compiler (host code only is run; no sanitizer here) and
run.  No GPU."""
import os
import subprocess

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)


def test_blocks_selftest(tmp_path):
    import slam.net_amd.build as b
    exe = str(tmp_path / "blocks_selftest")
    cmd = [b.hipcc(), "--offload-arch=gfx950", "-std=c++17", "-O1", "-Wall", "-Werror", "-Wno-unused-function",
           "-I", b.CSRC, "-I", os.path.join(ROOT, "include"), os.path.join(HERE, "blocks_selftest.hip"), "-o", exe]
    r = subprocess.run(cmd, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, timeout=600)
    assert r.returncode == 0, r.stdout.decode(errors="replace")
    r = subprocess.run([exe], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, timeout=120)
    out = r.stdout.decode(errors="replace")
    assert r.returncode == 0 and out.startswith("ok: "), out
