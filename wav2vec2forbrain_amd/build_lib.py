"""Builds libb2p_hip.so (the C-ABI HIP library) in-tree with hipcc for gfx950.

Each csrc/*.hip / *.cpp file is compiled to an object under build/ and linked into
wav2vec2forbrain_amd/libb2p_hip.so. Staleness is decided by content, not by mtime: every object
carries a SHA-256 stamp of its source, the csrc/*.inc templates it includes, every header and the
compiler flags (`<obj>.sha`), and the library carries the hash of all of them
(`libb2p_hip.so.sha`). A library whose stamp matches the sources is current whatever the file times
say (a snapshot copied to the GPU box keeps the .so and its stamp); one whose stamp differs is
rebuilt even when it is newer than an edited source. The library links only the HIP runtime, by
SONAME (libamdhip64.so.7), so inside a process that imported torch it binds to the runtime torch
already loaded.
"""
from __future__ import annotations

import concurrent.futures as cf
import glob
import os
import subprocess
import sys

PKG = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(PKG)
CSRC = os.path.join(PKG, "csrc")
BUILD = os.path.join(ROOT, "build", "obj")
LIB = os.path.join(PKG, "libb2p_hip.so")
HIPCC = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
ARCH = "gfx950"
FLAGS = ["-O3", "-std=c++17", "-fPIC", f"--offload-arch={ARCH}", "-munsafe-fp-atomics",
         "-Wno-unused-result"]
# per-source codegen flags (none at present). Tried and reverted: attn16.hip with -mllvm
# -amdgpu-mfma-vgpr-form=1 (no v_accvgpr_read of the score / output accumulators, 84 fewer VALU
# instructions per forward tile) ran the forward 32.3 -> 34.1 us.
EXTRA_FLAGS: dict = {}


LIB_STAMP = LIB + ".sha"


def _read(path: str) -> bytes:
    with open(path, "rb") as f:
        return f.read()


def _headers_hash() -> str:
    import hashlib
    h = hashlib.sha256()
    for p in sorted(glob.glob(os.path.join(CSRC, "*.h")) + glob.glob(os.path.join(ROOT, "include", "*.h"))):
        h.update(os.path.basename(p).encode() + b"\0" + _read(p))
    return h.hexdigest()


def _src_hash(src: str, hh: str) -> str:
    """Stamp of one object: its source, the csrc/*.inc kernel templates it includes (shared by several
    instantiation units: only their includers rebuild when they change), every header, the flags."""
    import hashlib
    import re
    h = hashlib.sha256(" ".join([HIPCC, *FLAGS, *EXTRA_FLAGS.get(os.path.basename(src), [])]).encode() + hh.encode())
    text = _read(src)
    h.update(text)
    for name in re.findall(rb'#include "([^"]+\.inc)"', text):
        f = os.path.join(CSRC, name.decode())
        if os.path.exists(f):
            h.update(_read(f))
    return h.hexdigest()


def _stamp(path: str) -> str:
    try:
        return open(path).read().strip()
    except OSError:
        return ""


def _compile(src: str, sh: str, verbose: bool) -> str:
    obj = os.path.join(BUILD, os.path.basename(src) + ".o")
    if os.path.exists(obj) and _stamp(obj + ".sha") == sh:
        return obj
    cmd = [HIPCC, *FLAGS, *EXTRA_FLAGS.get(os.path.basename(src), []), "-c", src, "-o", obj]
    audit = os.environ.get("B2P_BUILD_AUDIT") == "1"
    if audit:   # per-kernel resource usage (VGPRs, LDS, scratch) saved beside the object
        cmd.append("-Rpass-analysis=kernel-resource-usage")
    if verbose:
        print(f"build_lib: hipcc {os.path.basename(src)}", file=sys.stderr, flush=True)
    r = subprocess.run(cmd, capture_output=True, text=True)
    if r.returncode != 0:
        raise RuntimeError(f"hipcc failed for {src}:\n{r.stdout}\n{r.stderr}")
    if audit:
        with open(obj + ".audit", "w") as f:
            f.write(r.stdout + r.stderr)
    with open(obj + ".sha", "w") as f:
        f.write(sh + "\n")
    return obj


def build(verbose: bool = False, jobs: int | None = None) -> str:
    """Compiles what is stale and links the library. Serialised across processes by a file lock
    (N bench ranks or a pytest run may call it at once on the same tree)."""
    import fcntl
    import time
    os.makedirs(BUILD, exist_ok=True)
    with open(os.path.join(BUILD, ".lock"), "w") as lk:
        fcntl.flock(lk, fcntl.LOCK_EX)
        t0 = time.perf_counter()
        path = _build_locked(verbose, jobs)
        if verbose:
            print(f"build_lib: {path} ready in {time.perf_counter() - t0:.1f} s", file=sys.stderr, flush=True)
        return path


def ensure_built() -> str:
    """The hook every GPU entry point (tests/conftest.py, bench.py, __graft_entry__.smoke) runs before
    its first HIP call: the committed tree carries sources only (the .so is git-ignored), so a fresh
    checkout builds here. Compilation runs in hipcc child processes; nothing here touches the GPU.
    A current library is returned without writing anything (no build/ directory, no lock file), so a
    tree that another user built and this one may only read still runs."""
    if _current(*_stamps()):
        return LIB
    return build(verbose=True)


def _stamps():
    """(sources, their stamps, the library's stamp) for the tree as it is."""
    import hashlib
    srcs = sorted(glob.glob(os.path.join(CSRC, "*.hip")) + glob.glob(os.path.join(CSRC, "*.cpp")))
    hh = _headers_hash()
    shas = [_src_hash(s, hh) for s in srcs]
    lib_sha = hashlib.sha256("".join(os.path.basename(s) + ":" + h + ";" for s, h in zip(srcs, shas)).encode()).hexdigest()
    return srcs, shas, lib_sha


def _current(srcs, shas, lib_sha) -> bool:
    # a library whose stamp matches is current even without the objects (a snapshot that carries the
    # built .so but not build/)
    return os.path.exists(LIB) and _stamp(LIB_STAMP) == lib_sha


def _build_locked(verbose: bool, jobs: int | None) -> str:
    srcs, shas, lib_sha = _stamps()
    if _current(srcs, shas, lib_sha):
        return LIB
    # the GPU box reports the whole machine's CPUs; its share is 16
    jobs = jobs or min(16, os.cpu_count() or 4)
    with cf.ThreadPoolExecutor(max_workers=jobs) as ex:
        objs = list(ex.map(lambda a: _compile(a[0], a[1], verbose), zip(srcs, shas)))
    tmp = LIB + ".tmp"
    cmd = [HIPCC, f"--offload-arch={ARCH}", "-shared", "-fPIC", "-o", tmp, *objs]
    if verbose:
        print(" ".join(cmd), file=sys.stderr, flush=True)
    r = subprocess.run(cmd, capture_output=True, text=True)
    if r.returncode != 0:
        raise RuntimeError(f"link failed:\n{r.stdout}\n{r.stderr}")
    os.replace(tmp, LIB)
    with open(LIB_STAMP, "w") as f:
        f.write(lib_sha + "\n")
    return LIB


if __name__ == "__main__":
    print(build(verbose="-v" in sys.argv))


def parse_scratch(text: str) -> dict:
    """{kernel: scratch_bytes_per_lane} from hipcc -Rpass-analysis=kernel-resource-usage output. A
    nonzero value means registers spilled or a private array went to scratch (e.g. accumulators
    indexed dynamically) — a silent 4x slowdown seen once."""
    import re
    out, cur = {}, None
    for line in text.splitlines():
        m = re.search(r"Function Name: (\S+)", line)
        if m:
            cur = m.group(1)
        m = re.search(r"ScratchSize \[bytes/lane\]: (\d+)", line)
        if m and cur:
            out[cur] = int(m.group(1))
    return out


def audit_scratch(src: str = "gemm.hip") -> dict:
    """Compiles one source with the resource-usage remarks and returns parse_scratch of them."""
    path = os.path.join(CSRC, src)
    r = subprocess.run([HIPCC, *FLAGS, "-c", path, "-o", os.devnull, "-Rpass-analysis=kernel-resource-usage"],
                       capture_output=True, text=True)
    return parse_scratch(r.stdout + r.stderr)
