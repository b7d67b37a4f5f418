"""What the CPU tests read from the gfx950 code object of the library in place: tools/kernel_regs.py's kernel_table,
loaded by path, so that the reader of the code-object metadata stands once."""
import importlib.util
import os
import re

_spec = importlib.util.spec_from_file_location(
    "kernel_regs", os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tools", "kernel_regs.py"))
_regs = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(_regs)
LLVM = _regs.LLVM


def binutils():
    """llvm-objdump and llvm-readelf stand beside the hipcc that built the library"""
    return os.path.exists(f"{LLVM}/llvm-objdump") and os.path.exists(f"{LLVM}/llvm-readelf")


def kernels(pattern):
    """{mangled name: (VGPRs, bytes of scratch)} of the library's kernels whose name matches the regular expression"""
    from neural_spectral_codec_amd import build
    return {k: (v["vgpr"], v["scratch"]) for k, v in _regs.kernel_table(build.LIB).items() if re.search(pattern, k)}
