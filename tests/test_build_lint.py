"""The build's ISA lint (sudo_rm_rf_amd/build.py): objects containing the packed-fp32 operand form that is wrong on
gfx950 next to MFMAs (op_sel = 1 on src1; tools/probes/pk_opsel_probe.hip) are refused.  CPU-only: the lint is a text
scan of the device assembly hipcc leaves behind.  Below it: source-level lints of the diagnostics switches (names, not numbers)
and of where cross-file functions are declared."""
import os
import re

from sudo_rm_rf_amd import build

BAD = """
	v_pk_add_f32 v[46:47], v[46:47], s[40:41] op_sel:[0,1]
	v_pk_mul_f32 v[0:1], v[74:75], v[54:55] op_sel:[0,1] op_sel_hi:[0,0]
	v_pk_fma_f32 v[4:5], v[2:3], v[70:71], v[30:31] op_sel:[0,1,0] op_sel_hi:[1,0,1]
"""
GOOD = """
	v_pk_mul_f32 v[2:3], v[26:27], v[74:75] op_sel_hi:[1,0]
	v_pk_fma_f32 v[82:83], s[4:5], v[44:45], v[82:83] op_sel:[1,0,0]
	v_pk_fma_f32 v[40:41], v[70:71], v[0:1], v[110:111] op_sel:[0,0,1] op_sel_hi:[0,1,0] neg_lo:[1,0,0] neg_hi:[1,0,0]
	v_pk_add_f32 v[8:9], v[8:9], v[10:11] op_sel_hi:[1,0]
	v_cvt_pk_bf16_f32 v3, v0, v1
	; v_pk_add_f32 v[0:1], v[0:1], v[2:3] op_sel:[0,1]   (a comment is not an instruction)
"""


def test_lint_flags_src1_op_sel(tmp_path):
    p = tmp_path / "bad.s"
    p.write_text(BAD)
    hits = build.isa_lint(str(p))
    assert [h[0] for h in hits] == [2, 3, 4]


def test_lint_accepts_safe_forms(tmp_path):
    p = tmp_path / "good.s"
    p.write_text(GOOD)
    assert build.isa_lint(str(p)) == []


def test_every_source_is_listed_and_gemm_files_build_without_slp():
    listed = set(build.SOURCES)
    on_disk = {f for f in os.listdir(build.CSRC) if f.endswith(".hip")}
    assert listed == on_disk, (listed ^ on_disk)
    for f in ("srf_pwconv_bf16x3.hip", "srf_pwconv_wgrad.hip"):
        assert "-fno-slp-vectorize" in build.FILE_FLAGS[f]


# ---- the diagnostics switches have names, and cross-file entry points are declared in headers only -------------------------------
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _header_debug_flags():
    """{name without SRF_DBG_: value as an unsigned 32-bit number} of enum srf_debug_flag, parsed as text."""
    text = open(os.path.join(ROOT, "include", "sudormrf_hip.h")).read()
    body = re.search(r"enum srf_debug_flag \{(.*?)\};", text, re.S).group(1)
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    out = {}
    for item in filter(None, (i.strip() for i in body.split(","))):
        name, expr = (s.strip() for s in item.split("="))
        assert name.startswith("SRF_DBG_") and re.fullmatch(r"[-0-9 <()]+", expr), item
        out[name[len("SRF_DBG_"):]] = eval(expr) & 0xFFFFFFFF
    return out


def test_debug_flag_enum_is_one_bit_per_name_and_python_mirrors_it():
    from sudo_rm_rf_amd import ops
    flags = _header_debug_flags()
    assert len(flags) == 32 and len(set(flags.values())) == 32
    assert all(v and v & (v - 1) == 0 for v in flags.values()), flags
    assert {m.name: int(m.value) for m in ops.DebugFlag} == flags


def test_debug_flag_values_bench_relies_on_keep_their_meaning():
    """bench.py tests --debug-flags against these numbers, tools/gpu_ab.sh passes them on its command line."""
    flags = _header_debug_flags()
    want = {"NO_PAIRS": 1, "NO_GEMM_256": 4, "NO_PACKED_WEIGHTS": 8, "PYR_PER_LEVEL": 16, "TRAIN_BF16X3": 16384,
            "NO_FUSED_TAIL": 32768, "BWD_NO_FUSED_HEAD": 1 << 16, "BWD_DW_CHUNKED": 1 << 29, "BWD_GLN_SCALAR": 1 << 30}
    assert {k: flags.get(k) for k in want} == want


_NUM = r"\(*\s*(?:\(\s*unsigned\s*\)\s*)?(?:0[xX][0-9a-fA-F]+|\d+)"


def test_no_source_tests_the_debug_flags_against_a_number():
    bad = []
    for f in sorted(os.listdir(build.CSRC)):
        if f.endswith((".hip", ".h")):
            for i, line in enumerate(open(os.path.join(build.CSRC, f)), 1):
                code = line.split("//")[0]
                if re.search(r"(srf_debug_flags\(\)|\bflags)\s*&\s*" + _NUM, code) or re.search(r"\bsrf_dbg\(\s*" + _NUM, code):
                    bad.append("%s:%d: %s" % (f, i, line.strip()))
    assert not bad, "\n".join(bad)


def test_no_test_or_tool_passes_a_numeric_debug_flag():
    bad = []
    for top in ("tests", "tools"):
        for d, dirs, files in os.walk(os.path.join(ROOT, top)):
            dirs[:] = [x for x in dirs if not (top == "tools" and x == "lab") and x != "__pycache__"]
            for f in sorted(files):
                if f.endswith(".py"):
                    for i, line in enumerate(open(os.path.join(d, f), errors="replace"), 1):
                        m = re.search(r"\b(?:set_)?debug_flags\(\s*" + _NUM, line.split("#")[0])
                        if m and int(re.search(r"0[xX][0-9a-fA-F]+|\d+", m.group(0)).group(0), 0) != 0:
                            bad.append("%s:%d: %s" % (os.path.relpath(os.path.join(d, f), ROOT), i, line.strip()))
    assert not bad, "\n".join(bad)


def _file_scope_functions(src):
    """(declared, defined): names of the non-static functions a .hip declares (prototype) / defines at file scope."""
    src = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    src = re.sub(r"//[^\n]*", "", src)
    src = re.sub(r'"(?:\\.|[^"\\\n])*"', '""', src)
    src = re.sub(r"'(?:\\.|[^'\\\n])'", "' '", src)
    src = re.sub(r"^[ \t]*#(?:[^\n]*\\\n)*[^\n]*", "", src, flags=re.M)      # preprocessor lines
    declared, defined = [], set()
    depth = paren = 0
    seg = []
    for ch in src:
        if depth:
            depth += (ch == "{") - (ch == "}")
            continue
        paren += (ch == "(") - (ch == ")")
        if ch == "}":                  # end of an extern "C" / namespace block
            seg = []
        elif paren == 0 and ch in ";{":
            s = " ".join("".join(seg).split())
            seg = []
            if ch == "{" and re.fullmatch(r'extern ""|namespace( \w+)?', s):
                continue               # transparent: what it holds is at file scope
            m = re.match(r"([^()=]*?)\b(\w+) ?\(", s)
            if m and m.group(1).strip() and not s.startswith("template") and \
                    not re.search(r"\b(static|typedef|using|struct|class|enum|__global__)\b", m.group(1)):
                if ch == ";":
                    declared.append(m.group(2))
                else:
                    defined.add(m.group(2))
            depth = ch == "{"
        else:
            seg.append(ch)
    return declared, defined


def test_cross_file_entry_points_are_declared_in_headers_only():
    """A prototype inside a .hip is a forward declaration of a function that file defines itself; everything that crosses
    translation units is declared once, in srf_internal.h / srf_pw.h / srf_pyr.h or the public header."""
    declared, defined = _file_scope_functions('''
        #include "x.h"
        static int local(int a);                 // file-local forward declaration: fine
        int elsewhere(const float* p, int n = 3);
        extern "C" int public_thing(void* s);
        extern "C" int public_thing(void* s) { if (s) { return 1; } return elsewhere(0); }
        static std::atomic<int> g{0};
        __global__ void kern(int* p) { p[0] = 1; }
        bool here(int a) { return a; }
    ''')
    assert declared == ["elsewhere", "public_thing"] and defined == {"public_thing", "here"}      # (the scanner itself)
    bad = []
    for f in build.SOURCES:
        declared, defined = _file_scope_functions(open(os.path.join(build.CSRC, f)).read())
        bad += ["%s declares %s, which it does not define" % (f, n) for n in declared if n not in defined]
    assert not bad, "\n".join(bad)
    assert os.path.join(build.CSRC, "srf_internal.h") in build.HEADERS
