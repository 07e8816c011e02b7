"""What the CPU tests of the ctypes bindings share (tests/test_capi_cpu.py for qlamd.h, tests/test_plant_contacts_cpu.py,
test_contact_update_cpu.py, test_plant_friction_cpu.py and test_contact_anchor_cpu.py for the extension headers): the recorder
that stands in for the loaded library, the header parser, the layout program the C compiler answers, and the kernels' resources
against DESIGN.md.  The expectations themselves -- arities, sizes, bit values, register bounds -- stay in the test files."""
import ctypes as C
import os
import re
import subprocess

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INCLUDE = os.path.join(ROOT, "include")
GCC = ["gcc", "-std=c11", "-Wall", "-Wextra", "-pedantic", "-Werror", "-I" + INCLUDE]
GXX = ["g++", "-std=c++17", "-Wall", "-Wextra", "-pedantic", "-Werror", "-I" + INCLUDE]
PARAMETER_KINDS = {"int": C.c_int, "int64_t": C.c_int64, "double": C.c_double, "unsigned": C.c_uint}
RETURN_KINDS = {"int": C.c_int, "void": None, "unsigned": C.c_uint, "size_t": C.c_size_t, "const char *": C.c_char_p}


# ---- what the wrappers hand to an entry -------------------------------------------------------------------------------------------

class Recorder:
    """Stands in for the loaded library: every entry records its arguments as the entry would see them while the call is in
    progress -- scalars by value, structs read back member by member from the recorded byref -- and returns 0."""

    def __init__(self):
        self.calls = []

    def __getattr__(self, name):
        if not name.startswith("qlamd_"):
            raise AttributeError(name)

        def fn(*args):
            self.calls.append((name, [self.snap(v) for v in args]))
            return 0
        fn.__name__ = name
        return fn

    @staticmethod
    def snap(v):
        if hasattr(v, "_obj"):
            v = v._obj
        if isinstance(v, C.Structure):
            return {n: getattr(v, n) for n, _ in v._fields_}
        return v.value if isinstance(v, C._SimpleCData) else v


def p(a):
    if a is None:
        return None
    return a.data_ptr() if hasattr(a, "data_ptr") else a.ctypes.data


def f64(*shape):
    return np.arange(int(np.prod(shape)), dtype=np.float64).reshape(shape) + 1.0


# key of a state dict -> member of qlamd_wholebody_batch; member of qlamd_plant_next -> key
WB = dict(q="joint_position", qd="joint_velocity", base_quat="base_orientation", base_linvel="base_linear_velocity",
          base_angvel="base_angular_velocity", stance="support_leg", normals="surface_normal")
NEXT = (("joint_position", "q"), ("joint_velocity", "qd"), ("base_position", "base_pos"), ("base_orientation", "base_quat"),
        ("base_linear_velocity", "base_linvel"), ("base_angular_velocity", "base_angvel"))


# ---- a binding against its header and the compiler --------------------------------------------------------------------------------

def header_declarations(header):
    """[(return type, name, [parameter kind: "pointer" or a key of PARAMETER_KINDS], [parameter name])] of every function the
    header `header` (a path) declares, in its order."""
    text = re.sub(r"/\*.*?\*/", " ", open(header).read(), flags=re.S)
    out = []
    for ret, name, params in re.findall(r"^(int|void|unsigned|size_t|const char \*) ?(qlamd_\w+)\(([^;{]*)\);", text, flags=re.M):
        prms = [x.strip() for x in params.split(",") if x.strip() != "void"]
        out.append((ret, name, ["pointer" if "*" in prm else " ".join(prm.split()[:-1]) for prm in prms],
                    [prm.split()[-1].lstrip("*") for prm in prms]))
    return out


def header_structs(header):
    """the names of the structs the header defines"""
    return set(re.findall(r"^typedef struct (qlamd_\w+) \{", open(header).read(), flags=re.M))


def signatures_match(module, header, typed_pointers=False):
    """Every function `header` declares has its row in module.SIGNATURES, in the header's order, with the declaration's return
    kind, arity and kind of each parameter; a pointer is a c_void_p (typed_pointers: or a POINTER type).
    -> {name: [parameter name]}"""
    decls = header_declarations(header)
    assert [name for _, name, _, _ in decls] == list(module.EXPORTS) == list(module.SIGNATURES)
    for ret, name, kinds, _ in decls:
        restype, argtypes = module.SIGNATURES[name]
        assert restype is RETURN_KINDS[ret], name
        assert len(argtypes) == len(kinds), name
        for i, (t, kind) in enumerate(zip(argtypes, kinds)):
            if kind == "pointer":
                assert t is C.c_void_p or (typed_pointers and issubclass(t, C._Pointer)), (name, i)
            else:
                assert t is PARAMETER_KINDS[kind], (name, i, kind)
    return {name: names for _, name, _, names in decls}


def layout(header, structs, constants, where):
    """What the C compiler says about `header` (a path), asked by a program generated from the binding's own mirrors and
    constants: {"sizeof <struct>" | "sizeof <struct> <member>" | "offsetof <struct> <member>" | "value <NAME>": integer}.
    structs: {C name: ctypes mirror, or the list of member names to ask about}; constants: names without the QLAMD_ prefix;
    where: a directory for the program.  A member or a constant the header does not have does not compile."""
    lines = []
    for cname, cls in structs.items():
        lines.append('printf("sizeof %s %%zu\\n", sizeof(%s));' % (cname, cname))
        for member in ([f[0] for f in cls._fields_] if hasattr(cls, "_fields_") else cls):
            lines.append('printf("sizeof %s %s %%zu\\n", sizeof(((%s *)0)->%s));' % (cname, member, cname, member))
            lines.append('printf("offsetof %s %s %%zu\\n", offsetof(%s, %s));' % (cname, member, cname, member))
    lines += ['printf("value %s %%lld\\n", (long long)(QLAMD_%s));' % (n, n) for n in constants]
    src, exe = os.path.join(str(where), "layout.c"), os.path.join(str(where), "layout")
    with open(src, "w") as f:
        f.write('#include <stddef.h>\n#include <stdio.h>\n#include "%s"\nint main(void) {\n  %s\n  return 0;\n}\n'
                % (os.path.basename(header), "\n  ".join(lines)))
    subprocess.check_call(GCC + [src, "-o", exe])
    out = subprocess.run([exe], capture_output=True, text=True, check=True, timeout=60).stdout
    return {line.rsplit(" ", 1)[0]: int(line.rsplit(" ", 1)[1]) for line in out.splitlines()}


def mirrors_match(structs, got):
    """Each ctypes mirror of `structs` ({C name: class}) has the size, the member offsets and the member sizes of layout()'s answer."""
    for cname, cls in structs.items():
        assert C.sizeof(cls) == got["sizeof " + cname], cname
        for member, ctype in cls._fields_:
            assert getattr(cls, member).offset == got["offsetof %s %s" % (cname, member)], (cname, member)
            assert C.sizeof(ctype) == got["sizeof %s %s" % (cname, member)], (cname, member)


# ---- the kernels' resources -------------------------------------------------------------------------------------------------------

def resources(unit, kernels, count, where):
    """The kernels `kernels` of the unit `unit` (count kernels in all), compiled with the build's flags: each one's registers,
    private segment and LDS in the code-object metadata are the figures DESIGN.md states for it, and none has a private segment.
    -> {kernel: ([VGPR, AGPR, private segment, LDS], the kernel's instruction lines)}"""
    from tools import kernel_isa
    text = open(os.path.join(ROOT, "DESIGN.md")).read()
    path = kernel_isa.assemble(unit, out=os.path.join(str(where), unit.replace(".hip", ".s")))
    md, asm, body = kernel_isa.meta(path), open(path).read(), kernel_isa.kernels(path)
    assert len([k for k in md if "kernel" in k]) == len(re.findall(r"\.group_segment_fixed_size:", asm)) == count
    seen = {}
    for kernel in kernels:
        m = re.search(r"`%s`: (\d+) VGPR, (\d+) AGPR, (\d+) B private segment, (\d+) B LDS" % kernel, text)
        assert m, "DESIGN.md does not state the resources of %s" % kernel
        names = [k for k in md if kernel in k]
        assert len(names) == 1, kernel
        lds = re.search(r"\.group_segment_fixed_size:\s+(\d+)\n(?:(?!.*\.group_segment_fixed_size).*\n)*?\s+\.name:\s+%s\n" % re.escape(names[0]), asm)
        got = [md[names[0]]["vgpr"], md[names[0]].get("agpr", 0), md[names[0]].get("scratch", 0), int(lds.group(1))]
        assert got == [int(x) for x in m.groups()], (kernel, got)
        assert got[2] == 0, kernel
        seen[kernel] = (got, body[names[0]])
    return seen
