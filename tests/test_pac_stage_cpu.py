"""
CPU test of the pure parts of the `.pac` readers' host glue (mrcaudiocodec_amd/csrc/mrc_pac_stage.hpp): the staging layout
builder, the chunk locator and the block-kind counting.  tests/pac_stage_check.cpp compiles the header alone for the host --
with AddressSanitizer and UndefinedBehaviorSanitizer where g++ has them -- and holds each against values written out by
hand; it must exit clean and say nothing.
"""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SAN = ["-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-fno-omit-frame-pointer"]


def test_layout_locator_and_block_counts(tmp_path):
    src = os.path.join(ROOT, "tests", "pac_stage_check.cpp")
    exe = str(tmp_path / "pac_stage_check")
    probe = subprocess.run(["g++", "-x", "c++", "-", "-o", str(tmp_path / "probe")] + SAN,
                           input=b"int main() { return 0; }\n", capture_output=True)
    flags = SAN if probe.returncode == 0 else []
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Wextra"] + flags +
                          ["-I", os.path.join(ROOT, "mrcaudiocodec_amd", "csrc"), src, "-o", exe])
    run = subprocess.run([exe], capture_output=True, env=dict(os.environ, ASAN_OPTIONS="detect_leaks=1"))
    assert run.returncode == 0 and not run.stderr, run.stderr.decode(errors="replace")[-3000:]
    print("sanitizers %s" % ("on" if flags else "not available"))
