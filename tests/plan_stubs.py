"""Recording stubs for the launch plan (csrc/plan.hip), generated from include/diffusers_amd.h.

plan.hip is host code: `run_op` pulls every entry point's arguments out of 64-bit slots with hand-written casts that must agree,
slot by slot, with `kSig[]` and with the prototype.  Nothing in the compiler checks that, so tests/test_plan_marshalling_cpu.py links
plan.hip against one stub per DA_FN_* entry point instead of the kernels: each stub has exactly the header's prototype, appends every
argument (the stream included) to a log as (type class, 64-bit image) and returns a status the driver sets.  The stubs, the struct field
tables and the type classes all come from parsing the header -- a new DA_FN_* is covered the day it is added.

`DRIVER` is the `main` that goes with them: it reads a script of one command per line and prints what the stubs saw (`Harness.run`).

    kinds                      the DA_FN_* table as plan.hip sees it, sizeof / field tables of the parameter structs
    blob <i> <hex>             host object i (a parameter struct, a host array), in an allocation of exactly that size
    op <fn> <slot>...          append an op; a slot is a hex number or @<i> = the address of blob i
    create                     da_plan_create over the appended ops          -> "create <rc>"
    mutate                     flip every byte of every blob (the caller reusing its memory)
    status <fn> <rc>           what that entry point's stub returns from now on
    relocate (<old> <bytes> <new>)...                                        -> "relocate <rc> <unmatched>"
    launch <stream>            da_plan_launch                                -> "launch <rc> <failed_op>", one "call ..." per stub call
    destroy
"""
from __future__ import annotations

import re
import shutil
import subprocess
from pathlib import Path

ROOT = Path(__file__).resolve().parent.parent
HEADER = ROOT / "include" / "diffusers_amd.h"
PLAN_SRC = ROOT / "diffusers_amd" / "csrc" / "plan.hip"

CLASSES = {"pointer": "p", "int": "i", "long long": "l", "float": "f"}


def type_class(ctype: str) -> str:
    """'p' / 'i' / 'l' / 'f' of a C parameter or field type as the header spells it."""
    t = ctype.strip()
    if "*" in t:
        return "p"
    t = re.sub(r"\b(const|unsigned|signed)\b", "", t).strip()
    if t == "long long":
        return "l"
    if t == "int":
        return "i"
    if t == "float":
        return "f"
    raise ValueError(f"type {ctype!r} has no class")


def _split_decl(decl: str):
    """'const void* const* weight' -> ('const void* const*', 'weight')"""
    m = re.fullmatch(r"(.*?)(\w+)", re.sub(r"\[[^\]]*\]", "", decl).strip(), re.S)      # (an array member: its element type)
    return " ".join(m.group(1).split()), m.group(2)


def parse_header(text: str | None = None) -> dict:
    """{"fns": [(id, DA_FN_ macro, entry point)], "protos": {name: (return type, [(type, name)])}, "structs": {name: [(type, field)]},
    "defines": {name: int}} of the header."""
    text = HEADER.read_text() if text is None else text
    fns = [(int(m.group(2)), m.group(1), m.group(3)) for m in re.finditer(r"#define (DA_FN_\w+) (\d+)\s*/\* (da_\w+) \*/", text)]
    defines = {m.group(1): int(m.group(2)) for m in re.finditer(r"#define (DA_\w+) (-?\d+)\b", text)}
    code = re.sub(r"/\*.*?\*/", " ", text, flags=re.S)
    code = re.sub(r"^\s*#.*$", " ", code, flags=re.M)
    structs = {}
    for m in re.finditer(r"typedef struct (da_\w+) \{(.*?)\} \1;", code, re.S):
        fields = []
        for decl in m.group(2).split(";"):
            if not decl.strip():
                continue
            first, *more = decl.split(",")
            ctype, name = _split_decl(first)
            fields.append((ctype, name))
            fields += [(ctype, n.strip()) for n in more]               # `int M, N, K;` -- never used with pointer declarators here
        structs[m.group(1)] = fields
    code = re.sub(r"typedef struct (da_\w+) \{.*?\} \1;", " ", code, flags=re.S)
    protos = {}
    for m in re.finditer(r"([\w \*]+?)\b(da_\w+)\s*\(([^)]*)\)\s*;", code):
        params = [] if m.group(3).strip() in ("", "void") else [_split_decl(p) for p in m.group(3).split(",")]
        protos[m.group(2)] = (" ".join(m.group(1).split()), params)
    return {"fns": sorted(fns), "protos": protos, "structs": structs, "defines": defines}


def pointer_fields(doc: dict, struct: str) -> list:
    return [name for ctype, name in doc["structs"][struct] if "*" in ctype]


STRUCTS = {"da_gemm_params": "G", "da_attention_params": "A"}


def generate_stubs(doc: dict) -> str:
    """C++ source of the stubs and of the tables the driver prints."""
    out = ['// generated from include/diffusers_amd.h by tests/plan_stubs.py', '#include <cstddef>', '#include <cstring>', '#include <string>',
           '#include <vector>', '#include "diffusers_amd.h"', '',
           'struct LoggedArg { char cls; unsigned long long image; };',
           'struct LoggedCall {',
           '  int fn;',
           '  std::vector<LoggedArg> args;',
           '  std::vector<std::string> structs;          // the bytes of every parameter struct the call received',
           '  std::vector<long long> ints;                // host int array(s) of `parts` entries',
           '  std::vector<unsigned long long> ptrs;       // host pointer array(s) of `parts` entries',
           '};',
           'std::vector<LoggedCall> g_log;',
           'int g_status[DA_FN_COUNT];',
           '',
           '// the class is taken from the DECLARED type of the parameter: overload resolution on the header\'s own prototype',
           'static void note(LoggedCall& c, int v) { c.args.push_back({\'i\', (unsigned long long)(long long)v}); }',
           'static void note(LoggedCall& c, long long v) { c.args.push_back({\'l\', (unsigned long long)v}); }',
           'static void note(LoggedCall& c, float v) { unsigned u; std::memcpy(&u, &v, 4); c.args.push_back({\'f\', u}); }',
           'static void note(LoggedCall& c, const void* v) { c.args.push_back({\'p\', (unsigned long long)(size_t)v}); }',
           'template <class T> static void keep_struct(LoggedCall& c, const T* p) {',
           '  if (p) c.structs.emplace_back((const char*)p, sizeof(T));',
           '}', '']
    names = []
    for fid, macro, name in doc["fns"]:
        ret, params = doc["protos"][name]
        names.append((fid, macro, name))
        out.append(f'extern "C" {ret} {name}({", ".join(f"{t} {n}" for t, n in params)}) {{')
        out.append(f'  LoggedCall c; c.fn = {macro};')
        has_parts = any(n == "parts" and t == "int" for t, n in params)
        for t, n in params:
            out.append(f'  note(c, {n});')
            base = t.replace("const", "").replace("*", "").strip()
            if base in STRUCTS:
                out.append(f'  keep_struct(c, {n});')
            elif has_parts and t == "const int*":
                out.append(f'  for (int j = 0; j < parts; ++j) c.ints.push_back({n}[j]);')
            elif has_parts and t == "const void* const*":
                out.append(f'  for (int j = 0; j < parts; ++j) c.ptrs.push_back((unsigned long long)(size_t){n}[j]);')
        out.append(f'  g_log.push_back(c);')
        out.append(f'  return g_status[{macro}];')
        out.append('}')
    out.append('')
    out.append('const char* const kFnName[DA_FN_COUNT] = {')
    by_id = {fid: name for fid, _, name in names}
    for i in range(doc["defines"]["DA_FN_COUNT"]):
        out.append(f'    {"nullptr" if i not in by_id else chr(34) + by_id[i] + chr(34)},')
    out.append('};')
    out.append('struct FieldInfo { const char* owner; const char* name; size_t offset, size; int pointer; };')
    out.append('const FieldInfo kFields[] = {')
    for struct in STRUCTS:
        for ctype, name in doc["structs"][struct]:
            out.append(f'    {{"{struct}", "{name}", offsetof({struct}, {name}), sizeof((({struct}*)0)->{name}), {int("*" in ctype)}}},')
    out.append('    {nullptr, nullptr, 0, 0, 0}};')
    out.append('const size_t kStructSize[] = {' + ", ".join(f"sizeof({s})" for s in STRUCTS) + '};')
    out.append('const char* const kStructName[] = {' + ", ".join(f'"{s}"' for s in STRUCTS) + ', nullptr};')
    return "\n".join(out) + "\n"


DRIVER = r'''
// the driver: one command per line of the script named on the command line (see tests/plan_stubs.py)
#include <cstdio>
#include <cstdlib>
#include <fstream>
#include <iostream>
#include <memory>
#include <sstream>

static unsigned long long hex64(const std::string& s) { return std::strtoull(s.c_str(), nullptr, 16); }

int main(int argc, char** argv) {
  if (argc != 2) return 2;
  std::ifstream in(argv[1]);
  if (!in) return 2;
  std::vector<std::unique_ptr<unsigned char[]>> blobs;
  std::vector<size_t> blob_bytes;
  std::vector<da_plan_op> pending;
  da_plan* plan = nullptr;
  std::string line;
  while (std::getline(in, line)) {
    std::istringstream ss(line);
    std::string cmd;
    if (!(ss >> cmd)) continue;
    if (cmd == "kinds") {
      for (int fn = 1; fn < DA_FN_COUNT; ++fn)
        std::printf("kinds %d %s %s %d\n", fn, kFnName[fn] ? kFnName[fn] : "?", da_plan_arg_kinds(fn), da_plan_arg_count(fn));
      for (int s = 0; kStructName[s]; ++s) std::printf("sizeof %s %zu\n", kStructName[s], kStructSize[s]);
      for (const FieldInfo* f = kFields; f->owner; ++f)
        std::printf("field %s %s %zu %zu %d\n", f->owner, f->name, f->offset, f->size, f->pointer);
      std::printf("unknown %d %d %d\n", da_plan_arg_count(0), da_plan_arg_count(DA_FN_COUNT), da_plan_arg_kinds(DA_FN_COUNT) == nullptr);
    } else if (cmd == "blob") {
      size_t i;
      std::string hex;
      ss >> i >> hex;
      if (hex == "-") hex.clear();
      if (blobs.size() <= i) blobs.resize(i + 1), blob_bytes.resize(i + 1, 0);
      blobs[i].reset(new unsigned char[hex.size() / 2]);
      blob_bytes[i] = hex.size() / 2;
      for (size_t b = 0; b < hex.size() / 2; ++b) blobs[i][b] = (unsigned char)std::strtoul(hex.substr(2 * b, 2).c_str(), nullptr, 16);
    } else if (cmd == "op") {
      da_plan_op op;
      std::memset(&op, 0, sizeof(op));
      ss >> op.fn;
      std::string tok;
      for (int a = 0; a < DA_PLAN_MAX_ARGS && (ss >> tok); ++a)
        op.arg[a] = tok[0] == '@' ? (unsigned long long)(size_t)blobs.at(std::strtoul(tok.c_str() + 1, nullptr, 10)).get() : hex64(tok);
      pending.push_back(op);
    } else if (cmd == "create") {
      if (plan) da_plan_destroy(plan);
      plan = nullptr;
      const int rc = da_plan_create(pending.empty() ? nullptr : pending.data(), (int)pending.size(), &plan);
      std::printf("create %d %d\n", rc, plan ? da_plan_op_count(plan) : -1);
      pending.clear();
    } else if (cmd == "mutate") {
      for (size_t i = 0; i < blobs.size(); ++i)
        for (size_t b = 0; b < blob_bytes[i]; ++b) blobs[i][b] ^= 0xFF;
    } else if (cmd == "status") {
      int fn, rc;
      ss >> fn >> rc;
      g_status[fn] = rc;
    } else if (cmd == "relocate") {
      std::vector<const void*> old_base;
      std::vector<unsigned long long> bytes;
      std::vector<void*> new_base;
      std::string a, b, c;
      while (ss >> a >> b >> c) {
        old_base.push_back((const void*)(size_t)hex64(a));
        bytes.push_back(hex64(b));
        new_base.push_back((void*)(size_t)hex64(c));
      }
      int miss = -1;
      const int rc = da_plan_relocate(plan, (int)bytes.size(), old_base.data(), bytes.data(), new_base.data(), &miss);
      std::printf("relocate %d %d\n", rc, miss);
    } else if (cmd == "launch") {
      std::string st;
      ss >> st;
      g_log.clear();
      int failed = -7;
      const int rc = da_plan_launch(plan, (void*)(size_t)hex64(st), &failed);
      std::printf("launch %d %d\n", rc, failed);
      for (const LoggedCall& c : g_log) {
        std::printf("call %s args=", kFnName[c.fn]);
        for (size_t i = 0; i < c.args.size(); ++i) std::printf("%s%c:%llx", i ? "," : "", c.args[i].cls, c.args[i].image);
        std::printf(" structs=");
        for (size_t i = 0; i < c.structs.size(); ++i) {
          if (i) std::printf("|");
          for (unsigned char ch : c.structs[i]) std::printf("%02x", ch);
        }
        std::printf(" ints=");
        for (size_t i = 0; i < c.ints.size(); ++i) std::printf("%s%lld", i ? "," : "", c.ints[i]);
        std::printf(" ptrs=");
        for (size_t i = 0; i < c.ptrs.size(); ++i) std::printf("%s%llx", i ? "," : "", c.ptrs[i]);
        std::printf("\n");
      }
    } else if (cmd == "destroy") {
      if (plan) da_plan_destroy(plan);
      plan = nullptr;
    } else {
      std::printf("bad command %s\n", cmd.c_str());
      return 3;
    }
  }
  if (plan) da_plan_destroy(plan);
  return 0;
}
'''


def find_hipcc():
    hipcc = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    return hipcc if Path(hipcc).exists() else None


class Harness:
    """plan.hip + the generated stubs + DRIVER as one stand-alone executable under `workdir`."""

    def __init__(self, workdir: Path, sanitize: bool = False, plan_src: Path = PLAN_SRC, header: Path = HEADER):
        self.dir = Path(workdir)
        self.dir.mkdir(parents=True, exist_ok=True)
        self.doc = parse_header(Path(header).read_text())
        src = self.dir / "harness.hip"
        src.write_text(generate_stubs(self.doc) + DRIVER)
        self.exe = self.dir / "plan_harness"
        cmd = [find_hipcc(), "--offload-arch=gfx950", "-O1", "-g", f"-I{Path(header).parent}", f"-I{Path(plan_src).parent}",
               str(plan_src), str(src), "-o", str(self.exe)]
        if sanitize:
            cmd[2:2] = ["-Xarch_host", "-fsanitize=address,undefined", "-Xarch_host", "-fno-omit-frame-pointer"]
        r = subprocess.run(cmd, capture_output=True, text=True)
        if r.returncode != 0:
            raise RuntimeError(f"{' '.join(cmd)}\n{r.stdout[-3000:]}{r.stderr[-3000:]}")
        self._n = 0

    def run(self, script: list) -> list:
        """Run the script; the output lines, split into words.  Any sanitizer report, any output on stderr and any non-zero exit
        status is an error."""
        self._n += 1
        path = self.dir / f"script{self._n}.txt"
        path.write_text("\n".join(script) + "\n")
        r = subprocess.run([str(self.exe), str(path)], capture_output=True, text=True, timeout=120)
        assert r.returncode == 0 and r.stderr == "", f"exit status {r.returncode}\n{r.stdout[-2000:]}\n{r.stderr[-4000:]}"
        return [ln.split() for ln in r.stdout.splitlines()]


def parse_call(words: list) -> dict:
    """A `call` line of the driver -> {"name", "args": [(class, image)], "structs": [bytes], "ints": [int], "ptrs": [int]}"""
    assert words[0] == "call"
    kv = dict(w.split("=", 1) for w in words[2:])
    return {"name": words[1],
            "args": [(a.split(":")[0], int(a.split(":")[1], 16)) for a in kv["args"].split(",") if a],
            "structs": [bytes.fromhex(s) for s in kv["structs"].split("|") if s],
            "ints": [int(v) for v in kv["ints"].split(",") if v],
            "ptrs": [int(v, 16) for v in kv["ptrs"].split(",") if v]}
