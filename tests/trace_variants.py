"""The trace-kernel instantiations compiled into libpt_hip.so, read from the library's gfx950 code objects (no GPU needed).

  llvm-objcopy          dumps the .hip_fatbin section: one offload bundle per translation unit, each starting with the magic
                        __CLANG_OFFLOAD_BUNDLE__
  clang-offload-bundler unbundles the gfx950 code object of each
  llvm-readelf -s       lists its kernel descriptors (<mangled name>.kd; .symtab and .dynsym both hold each one)

The template arguments are parsed out of the mangled names (Li<n>E, Lin<n>E for -n, Lb0E / Lb1E) in the argument order of
the templates (csrc/pt_kernels.h, csrc/pt_kernel_q.h):
  trace_kernel<LDS_SCENE, PRUNE, STATS, LIST>
  trace_kernel_v2<RES, PRUNE, STATS, THRESH, INNER, MINW, SPEC, NEE, LIST>
  trace_kernel_q<RES, STATS, SPEC, POSTPONE>
and packed the way info "trace_variant" reports the kernel a render launched (include/pt_api.h)."""
import os
import re
import subprocess
import tempfile
from collections import namedtuple

LLVM_BIN = os.path.join(os.environ.get("ROCM_PATH", "/opt/rocm"), "llvm", "bin")
ARCH = "gfx950"
BUNDLE_MAGIC = b"__CLANG_OFFLOAD_BUNDLE__"

FAMILIES = {"trace_kernel": 1, "trace_kernel_v2": 2, "trace_kernel_q": 3}
TEMPLATE_ARGS = {
    1: ("res", "prune", "stats", "list"),                     # res = LDS_SCENE
    2: ("res", "prune", "stats", "thresh", "inner", "minw", "spec", "nee", "list"),
    3: ("res", "stats", "spec", "postpone"),
}
FIELDS = ("family", "res", "prune", "stats", "spec", "nee", "list", "postpone", "thresh", "inner", "minw")


class Variant(namedtuple("Variant", FIELDS)):
    """One trace-kernel instantiation; a field the family's template does not have is 0."""
    __slots__ = ()

    @property
    def code(self):
        """The packing of info "trace_variant" (include/pt_api.h)."""
        return (self.family | self.res << 4 | int(self.prune) << 6 | int(self.stats) << 7 | self.spec << 8 |
                int(self.nee) << 10 | int(self.list) << 11 | int(self.postpone) << 12 | self.thresh << 16 |
                (self.inner & 0xFFFF) << 24 | self.minw << 40)

    @classmethod
    def decode(cls, code):
        inner = (code >> 24) & 0xFFFF
        return cls(family=code & 0xF, res=(code >> 4) & 3, prune=(code >> 6) & 1, stats=(code >> 7) & 1,
                   spec=(code >> 8) & 3, nee=(code >> 10) & 1, list=(code >> 11) & 1, postpone=(code >> 12) & 1,
                   thresh=(code >> 16) & 0xFF, inner=inner - 0x10000 if inner & 0x8000 else inner, minw=(code >> 40) & 0xF)

    def __str__(self):
        name = {1: "trace_kernel", 2: "trace_kernel_v2", 3: "trace_kernel_q"}[self.family]
        args = [f"{k}={int(getattr(self, k))}" for k in TEMPLATE_ARGS[self.family]]
        return f"{name}<{', '.join(args)}>"


_ARG = re.compile(r"L([ib])(n?)(\d+)E")


def parse_kernel_name(sym):
    """Variant of a mangled trace-kernel symbol (with or without the .kd suffix), None for any other symbol."""
    if not sym.startswith("_Z"):
        return None
    pos = 3 if sym.startswith("_ZN") else 2              # a nested name: namespace components, then the kernel's
    name = ""
    while True:
        m = re.compile(r"\d+").match(sym, pos)
        if not m:
            break
        n = int(m.group(0))
        name, pos = sym[m.end(): m.end() + n], m.end() + n
    rest = sym[pos:]
    if name not in FAMILIES or not rest.startswith("I"):
        return None
    family = FAMILIES[name]
    vals, pos = [], 1
    while True:
        a = _ARG.match(rest, pos)
        if not a:
            break
        vals.append(-int(a.group(3)) if a.group(2) else int(a.group(3)))
        pos = a.end()
    if rest[pos: pos + 1] != "E" or len(vals) != len(TEMPLATE_ARGS[family]):
        raise ValueError(f"cannot parse the template arguments of {sym}")
    fields = dict.fromkeys(FIELDS, 0)
    fields.update(zip(TEMPLATE_ARGS[family], vals), family=family)
    return Variant(**fields)


def _tool(name):
    return os.path.join(LLVM_BIN, name)


def _run(cmd):
    return subprocess.run(cmd, check=True, stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True).stdout


def code_object_symbols(lib_path):
    """Per offload bundle of the library: the set of kernel-descriptor symbols (without .kd) of its gfx950 code object."""
    out = []
    with tempfile.TemporaryDirectory() as tmp:
        fatbin = os.path.join(tmp, "fatbin")
        _run([_tool("llvm-objcopy"), "--dump-section", f".hip_fatbin={fatbin}", lib_path, os.path.join(tmp, "stripped")])
        with open(fatbin, "rb") as f:
            blob = f.read()
        starts = [m.start() for m in re.finditer(re.escape(BUNDLE_MAGIC), blob)]
        if not starts:
            raise RuntimeError(f"{lib_path}: no offload bundle in .hip_fatbin")
        for k, s in enumerate(starts):
            part = os.path.join(tmp, f"bundle{k}")
            with open(part, "wb") as f:
                f.write(blob[s: starts[k + 1] if k + 1 < len(starts) else len(blob)])
            targets = [t for t in _run([_tool("clang-offload-bundler"), "--list", "--type=o", f"--input={part}"]).split()
                       if t.endswith("--" + ARCH)]
            if len(targets) != 1:
                raise RuntimeError(f"bundle {k} of {lib_path}: {len(targets)} {ARCH} code objects")
            co = part + ".co"
            _run([_tool("clang-offload-bundler"), "--unbundle", "--type=o", f"--targets={targets[0]}", f"--input={part}",
                  f"--output={co}"])
            syms = set()
            for line in _run([_tool("llvm-readelf"), "-s", "--wide", co]).splitlines():
                cols = line.split()
                if cols and cols[-1].endswith(".kd"):
                    syms.add(cols[-1][:-3])
            out.append(syms)
    return out


def compiled_trace_variants(lib_path):
    """[(Variant, mangled name)] of every trace kernel in the library's gfx950 code objects: one entry per code object that
    holds the kernel, so a kernel compiled into two translation units appears twice."""
    found = []
    for syms in code_object_symbols(lib_path):
        for s in sorted(syms):
            v = parse_kernel_name(s)
            if v is not None:
                found.append((v, s))
    return found
