"""ASan + UBSan over the Python-free parts of the native edge
(ops/csrc/edge_pack.hpp): the lane split, the hot-lane packing and the
response framing, driven by the stand-alone csrc/edge_pack_driver.cpp over a
few hundred synthetic requests per batch. A sanitizer report or a mismatch
against the driver's per-row reference makes the binary exit non-zero."""

import subprocess
from pathlib import Path

BUILD = Path(__file__).resolve().parent.parent / "mcp_context_forge_amd" / "ops"
CSRC = BUILD / "csrc"
SOURCES = ["edge_pack_driver.cpp", "edge_pack.hpp"]


def _build() -> Path:
    out = BUILD / "san_driver_edge_pack"
    newest = max((CSRC / s).stat().st_mtime for s in SOURCES)
    if out.exists() and out.stat().st_mtime > newest:
        return out
    cmd = ["g++", "-O1", "-g", "-std=c++17", "-fsanitize=address,undefined",
           "-fno-sanitize-recover=undefined", "-fno-omit-frame-pointer",
           "-o", str(out), str(CSRC / "edge_pack_driver.cpp")]
    subprocess.run(cmd, check=True, capture_output=True, text=True)
    return out


def test_edge_pack_under_asan_ubsan():
    binary = _build()
    env = {"ASAN_OPTIONS": "detect_leaks=1:abort_on_error=0", "UBSAN_OPTIONS": "print_stacktrace=1"}
    r = subprocess.run([str(binary), "600", "6"], capture_output=True, text=True, timeout=120, env=env)
    assert r.returncode == 0, f"sanitizer:\n{r.stdout[-2000:]}\n{r.stderr[-4000:]}"
    assert "edge pack driver ok" in r.stdout
