"""The builder of the stand-alone host check programs (tests/*_check.cpp): a header of rend3_amd/csrc that the kernels share with the
host is compiled with a `main` of its own and run as a child process, on the CPU alone."""
import os
import shutil
import subprocess

BUILD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "_build")
SANITIZERS = ["-Xarch_host", "-fsanitize=address", "-Xarch_host", "-fsanitize=undefined", "-fno-sanitize-recover=all"]


def program(source, deps, *, sanitize=True, fp_contract_off=False):
    """Path of the program built from `source` (built once, and again when it or one of `deps` is newer).  sanitize: with the address
    and undefined-behaviour sanitizers, whose reports go to stderr; without them the program has a name of its own, for the callers
    that run it beside the GPU.  fp_contract_off: every f32 operation rounds once, as in the library's build."""
    out = os.path.join(BUILD, os.path.splitext(os.path.basename(source))[0] + ("" if sanitize else "_plain"))
    if not (os.path.exists(out) and os.path.getmtime(out) >= max(os.path.getmtime(f) for f in [source] + list(deps))):
        hipcc = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
        os.makedirs(BUILD, exist_ok=True)
        tmp = out + f".{os.getpid()}.tmp"
        flags = (["-ffp-contract=off"] if fp_contract_off else []) + ["-Wall", "-Werror"] + (SANITIZERS if sanitize else [])
        res = subprocess.run([hipcc, "-O1", "-g", "-std=c++17"] + flags + ["-o", tmp, "-x", "c++", source],
                             capture_output=True, text=True)  # (host code only: -x c++ makes no device pass)
        assert res.returncode == 0, os.path.basename(out) + " build failed:\n" + res.stdout + res.stderr
        os.replace(tmp, out)
    return out
