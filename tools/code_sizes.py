"""Per-kernel code size and instruction hash of the IMPC and dense QP kernels (cross-compile only, no GPU): the
device code of each translation unit that instantiates them (csrc/kernels/impc_kernel.hip, impc_store.hip,
impc_conn.hip, impc_fov.hip, impc_fov_est.hip; the kernels themselves are in the per-layout headers impc_dense.hpp,
impc_sep.hpp, impc_wide_kernels.hpp, impc_fov.hpp), of connectivity_control.hip and of the generic dense QP path
(csrc/dense_qp.hip) is compiled for gfx950 on its own
(--offload-device-only), and for every kernel symbol the table gives its size in bytes and the
SHA-1 of its disassembled instructions (mnemonics and operands; addresses and encodings dropped).
Two trees whose lines agree launch the same instructions for that kernel: the check that a change
left an existing instantiation alone.

    python tools/code_sizes.py [out.txt]
"""
import hashlib
import os
import re
import subprocess
import sys
import tempfile

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(REPO, "mpc-cbf_amd")
LLVM = "/opt/rocm/llvm/bin"
FLAGS = ["-O3", "-std=c++17", "-fPIC", "--offload-arch=gfx950", "-Wall", "-Wno-unused-function",
         "-munsafe-fp-atomics", "-mllvm", "-amdgpu-mfma-vgpr-form"]
SRCS = ["csrc/kernels/impc_kernel.hip", "csrc/kernels/impc_store.hip", "csrc/kernels/impc_conn.hip",
        "csrc/kernels/impc_fov.hip", "csrc/kernels/impc_fov_est.hip", "csrc/kernels/connectivity_control.hip",
        "csrc/dense_qp.hip", "csrc/kernels/team_rollout.hip"]


def device_code(src):
    """(symbol table, disassembly) of one source file's gfx950 code object."""
    with tempfile.TemporaryDirectory() as tmp:
        bundle, obj = os.path.join(tmp, "dev.bundle"), os.path.join(tmp, "dev.elf")
        subprocess.run(["/opt/rocm/bin/hipcc", *FLAGS, "--offload-device-only", "-c", src, "-o", bundle], cwd=PKG,
                       check=True)
        subprocess.run([f"{LLVM}/clang-offload-bundler", "--unbundle", "--type=o", f"--input={bundle}",
                        "--targets=hipv4-amdgcn-amd-amdhsa--gfx950", f"--output={obj}"], check=True)
        syms = subprocess.run([f"{LLVM}/llvm-readelf", "-sW", obj], check=True, capture_output=True, text=True).stdout
        dis = subprocess.run([f"{LLVM}/llvm-objdump", "-d", "--no-show-raw-insn", "--no-leading-addr", obj],
                             check=True, capture_output=True, text=True).stdout
    return syms, dis


def main():
    parts = [device_code(src) for src in SRCS if os.path.exists(os.path.join(PKG, src))]
    syms = "\n".join(p[0] for p in parts)
    dis = "\n".join(p[1] for p in parts)
    sizes = {}
    for ln in syms.splitlines():
        f = ln.split()
        if len(f) >= 8 and f[3] == "FUNC" and f[7].startswith("_ZN6mpccbf3dev"):
            sizes[f[7]] = int(f[2])  # (the symbol table lists a kernel twice: same size)
    body, cur = {}, None
    for ln in dis.splitlines():
        m = re.match(r"^<(\S+)>:", ln)
        if m:
            cur = m.group(1)
            body[cur] = []
        elif "file format" in ln or ln.startswith("Disassembly of section"):
            cur = None  # (the next object's header, with its temporary path: no kernel's instructions)
        elif cur is not None and ln.strip():
            body[cur].append(re.sub(r"\s*//.*$", "", ln.strip()))
    names = sorted(sizes)
    dem = subprocess.run(["c++filt"], input="\n".join(names), capture_output=True, text=True).stdout.splitlines()
    lines = [f"{'kernel':58s} {'code bytes':>10s}  instructions sha1"]
    for n, d in sorted(zip(names, dem), key=lambda t: t[1]):
        d = d.replace("mpccbf::dev::", "").split("(")[0].replace("void ", "")
        h = hashlib.sha1("\n".join(body.get(n, [])).encode()).hexdigest()[:16]
        lines.append(f"{d[:58]:58s} {sizes[n]:10d}  {h}")
    txt = "\n".join(lines) + "\n"
    if len(sys.argv) > 1:
        open(sys.argv[1], "w").write(txt)
    print(txt, end="")


if __name__ == "__main__":
    main()
