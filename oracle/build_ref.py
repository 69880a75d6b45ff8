"""Build the reference's own device code for the host: oracle/_ref/libemf_ref.so.

TEST INFRASTRUCTURE ONLY.  The reference (EmbodiedVision/emfusion) keeps its kernels in three CUDA
sources that are plain C++ apart from the ``kernel<<<grid, block, ...>>>(args)`` launch syntax.
This recipe reads them from the reference checkout (``EMF_REFERENCE_DIR``), rewrites every launch
into ``ref_launch(grid, block, kernel, args)`` (oracle/refshim/cuda_runtime.h: all blocks and
threads in a fixed order on one thread), writes the rewritten text to a temporary directory
OUTSIDE the repository, compiles it with oracle/ref_abi.cpp against the stand-in headers of
oracle/refshim/ and removes the temporary directory.  Only the shared library is left, under the
git-ignored oracle/_ref/.  No reference text, rewritten or not, is written where git looks.

Of the third source only kernel_computePoints, computePoints, fastpow and kernel_renderPhong are
compiled, cut out BY NAME: the rest of that file is host glue over OpenCV / thrust calls
(filterPoints, computePercentiles, renderGPU's lookup table) that has no kernel text to pin.

Pinned semantics: the reference source, IEEE single precision, no a*b+c contraction
(-ffp-contract=off) -- what oracle/emf_oracle.c and the product build claim.  nvcc's own choice of
where to contract cannot be reproduced on a CPU.
"""
from __future__ import annotations

import os
import re
import shutil
import subprocess
import sys
import tempfile
from pathlib import Path

HERE = Path(__file__).resolve().parent
OUT = HERE / "_ref" / "libemf_ref.so"
DEFAULT_REFERENCE = HERE.parent.parent / "reference"  # a checkout beside this repository
CXXFLAGS = ["-O2", "-std=c++17", "-ffp-contract=off", "-fPIC", "-shared"]

# kernel<<<grid, block[, shmem, stream]>>> (   ->   ref_launch(grid, block, kernel,
_LAUNCH = re.compile(r"(\w+(?:<\w+>)?)\s*<<<\s*(\w+)\s*,\s*(\w+)\s*(?:,[^>]*)?>>>\s*\(")
# launches each source must hold: a silent non-match would drop a kernel
_EXPECTED = {"TSDF.cu": 15, "ObjTSDF.cu": 1, "EMFusion.cu": 2}
# ref_launch runs threads one after another: nothing compiled may rely on anything else
_ORDER_DEPENDENT = re.compile(r"__shared__|__syncthreads|atomic[A-Z]\w*\s*\(|__shfl|__ballot|__syncwarp")
_EMFUSION_KEEP = ("kernel_computePoints", "computePoints", "fastpow", "kernel_renderPhong")


def reference_dir() -> Path:
    return Path(os.environ.get("EMF_REFERENCE_DIR", DEFAULT_REFERENCE))


def reference_present() -> bool:
    return (reference_dir() / "src" / "core" / "cuda" / "TSDF.cu").is_file()


def _rewrite(name: str, text: str, expected: int) -> str:
    out, n = _LAUNCH.subn(r"ref_launch(\2, \3, \1, ", text)
    if n != expected or "<<<" in out or ">>>" in out.replace(">>>=", ""):
        raise RuntimeError(f"{name}: rewrote {n} kernel launches, expected {expected}")
    bad = _ORDER_DEPENDENT.search(out)
    if bad:
        raise RuntimeError(f"{name}: '{bad.group(0)}' needs a real thread grid; ref_launch is serial")
    return out


def _definition(text: str, name: str) -> str:
    """The whole definition of function ``name``: qualifier lines above it through its closing brace."""
    m = re.search(r"^[ \t]*(?:[\w:<>]+[ \t]+)+" + re.escape(name) + r"[ \t]*\(", text, re.M)
    if not m:
        raise RuntimeError(f"EMFusion.cu: no definition of {name}")
    start = m.start()
    while True:  # qualifier-only lines (__global__, __host__ __device__, inline ...) directly above
        prev = text.rfind("\n", 0, start - 1) + 1
        line = text[prev:start].strip()
        if line and re.fullmatch(r"(?:(?:__\w+__|inline|static)\s*)+", line):
            start = prev
        else:
            break
    i = text.index("{", m.end())
    semi = text.find(";", m.end())
    if 0 <= semi < i:
        raise RuntimeError(f"EMFusion.cu: {name} matched a declaration, not a definition")
    depth = 0
    for j in range(i, len(text)):
        depth += text[j] == "{"
        depth -= text[j] == "}"
        if depth == 0:
            return text[start:j + 1]
    raise RuntimeError(f"EMFusion.cu: unbalanced braces in {name}")


def _cut_emfusion(text: str) -> str:
    head = text[:text.index("__global__")]  # the include and the namespace openers
    opened = head.count("{") - head.count("}")
    return head + "\n\n".join(_definition(text, n) for n in _EMFUSION_KEEP) + "\n" + "}\n" * opened


def build(verbose: bool = True) -> bool:
    """True: library built.  False: no reference tree here (an existing library is kept).  A
    reference tree that does not build raises."""
    ref = reference_dir()
    if not reference_present():
        if verbose:
            state = "kept" if OUT.exists() else "absent"
            print(f"oracle/build_ref: no reference tree at {ref}; oracle/_ref/libemf_ref.so {state}")
        return False
    tmp = Path(tempfile.mkdtemp(prefix="emf_ref_"))
    try:
        if HERE.parent in tmp.parents:
            raise RuntimeError("temporary directory lies inside the repository")
        for name in _EXPECTED:
            text = (ref / "src" / "core" / "cuda" / name).read_text()
            expected = _EXPECTED[name]
            if len(_LAUNCH.findall(text)) != expected or text.count("<<<") != expected:
                raise RuntimeError(f"{name}: expected {expected} kernel launches in the reference")
            if name == "EMFusion.cu":  # keeps computePoints' launch; ref_abi.cpp launches the Phong kernel
                text, expected = _cut_emfusion(text), 1
            (tmp / (Path(name).stem + "_host.inc")).write_text(_rewrite(name, text, expected))
        lib = tmp / OUT.name
        cmd = [os.environ.get("CXX", "g++"), *CXXFLAGS, f"-I{HERE / 'refshim'}", f"-I{ref / 'include'}",
               f"-I{tmp}", str(HERE / "ref_abi.cpp"), "-o", str(lib)]
        subprocess.run(cmd, check=True)
        OUT.parent.mkdir(exist_ok=True)
        shutil.copyfile(lib, OUT.with_suffix(".tmp"))
        os.replace(OUT.with_suffix(".tmp"), OUT)
    finally:
        shutil.rmtree(tmp, ignore_errors=True)
    if verbose:
        print(f"oracle/build_ref: built {OUT.relative_to(HERE.parent)} from {ref}")
    return True


if __name__ == "__main__":
    build()
    sys.exit(0)
