"""The launch plan's marshalling (csrc/plan.hip: kSig, run_op, for_each_device_pointer) against recording stubs, host only.

plan.hip is compiled with one generated stub per DA_FN_* entry point (tests/plan_stubs.py: prototypes, type classes and struct field
tables all parsed from include/diffusers_amd.h) into a stand-alone program; every check below drives that program with a script and
asserts what the stubs saw.  The program is built twice -- plain, and with the host AddressSanitizer / UBSan -- and every check runs on
both: the sanitizer build must exit 0 without a report.  No device, no installed library, no ctypes call into a stubbed function.

And the recorder's side of the same contract (diffusers_amd/plan.py): every launch entry point of the header is either replayable
(FN_IDS), reported as foreign when it runs under a recording (NOT_PLANNABLE), or passes through by design (PASS_THROUGH).
"""
import ctypes as C
import struct

import pytest

import plan_stubs as S

pytestmark = pytest.mark.skipif(S.find_hipcc() is None, reason="no hipcc")

DOC = S.parse_header()
FNS = DOC["fns"]                                   # [(id, macro, name)]
STREAM = 0x735700000040
INVALID, UNSUPPORTED = DOC["defines"]["DA_ERR_INVALID"], DOC["defines"]["DA_ERR_UNSUPPORTED"]
# two regions with different deltas, for da_plan_relocate: (old base, bytes, new base)
R0 = (0x7F1000000000, 0x10000, 0x7E2000000000)
R1 = (0x7F3000000000, 0x1000, 0x7D4000000000)
REGIONS = "relocate " + " ".join(f"{v:x}" for r in (R0, R1) for v in r)


def moved(v):
    for old, n, new in (R0, R1):
        if old <= v < old + n:
            return new + (v - old)
    return v


@pytest.fixture(scope="module", params=["plain", "sanitized"])
def harness(request, tmp_path_factory):
    return S.Harness(tmp_path_factory.mktemp(f"plan_{request.param}"), sanitize=request.param == "sanitized")


@pytest.fixture(scope="module")
def table(harness):
    return read_table(harness)


def read_table(harness):
    """What `kinds` prints: {"kinds": {fn: (name, letters)}, "sizeof": {struct: bytes}, "fields": {struct: [(name, offset, size, pointer)]}}"""
    out = {"kinds": {}, "sizeof": {}, "fields": {}}
    for w in harness.run(["kinds"]):
        if w[0] == "kinds":
            assert int(w[4]) == len(w[3])
            out["kinds"][int(w[1])] = (w[2], w[3])
        elif w[0] == "sizeof":
            out["sizeof"][w[1]] = int(w[2])
        elif w[0] == "field":
            out["fields"].setdefault(w[1], []).append((w[2], int(w[3]), int(w[4]), int(w[5])))
        else:
            assert w == ["unknown", "-1", "-1", "1"]
    SIZES.update(out["sizeof"])
    return out


def f32_bits(v):
    return struct.unpack("<I", struct.pack("<f", v))[0]


def u64(v):
    return v & 0xFFFFFFFFFFFFFFFF


def pattern(n, seed):
    return bytes((seed + 37 * i) & 0xFF for i in range(n))


def struct_of(letter):
    return {"G": "da_gemm_params", "A": "da_attention_params"}[letter]


def op_line(fid, slots):
    return f"op {fid} " + " ".join(s if isinstance(s, str) else f"{s:x}" for s in slots)


def calls_of(lines):
    return [S.parse_call(w) for w in lines if w[0] == "call"]


def params_of(name):
    return DOC["protos"][name][1]


# ---- the table itself ------------------------------------------------------------------------------------------------------------
def test_every_fn_has_a_prototype_and_its_letters_agree_with_the_header_types(table):
    assert [fid for fid, _, _ in FNS] == list(range(1, DOC["defines"]["DA_FN_COUNT"])) and len(FNS) == len(table["kinds"])
    for fid, _, name in FNS:
        got_name, kinds = table["kinds"][fid]
        params = params_of(name)
        assert got_name == name and DOC["protos"][name][0] == "int"
        assert params[-1] == ("void*", "stream"), name
        assert len(kinds) == len(params) - 1 <= DOC["defines"]["DA_PLAN_MAX_ARGS"], name
        for i, (k, (ctype, pname)) in enumerate(zip(kinds, params)):
            want = {"p": "pGAIQ", "i": "in", "l": "l", "f": "f"}[S.type_class(ctype)]
            assert k in want, f"{name} slot {i} ({ctype} {pname}): kSig says {k!r}"
            if k in "GA":
                assert struct_of(k) in ctype, f"{name} slot {i}"
            if k == "I":
                assert ctype == "const int*" and "n" in kinds[:i], f"{name} slot {i}"
            if k == "Q":
                assert ctype == "const void* const*" and "n" in kinds[:i], f"{name} slot {i}"


# ---- 1. slot values and order, every entry point -------------------------------------------------------------------------------
def slot_values(fid, kinds, blob0=0):
    """(slots, blob lines, expected image per slot or None for a host object) with a value per letter that only the right cast
    of run_op passes on unchanged."""
    slots, blobs, want, nb = [], [], [], blob0
    for i, k in enumerate(kinds):
        if k == "p":
            v = 0x5A00000000 | (fid << 20) | (i << 12) | 0x10           # distinct 40-bit addresses
        elif k == "i":
            v = u64(-(1000 + 17 * fid + i))                                # distinct negative ints
        elif k == "l":
            v = (1 << 40) + i
        elif k == "f":
            v = 0xDEADBEEF00000000 | f32_bits(i + 0.37)                    # "upper half ignored"
        elif k == "n":
            v = 3
        else:
            if k in "GA":
                data = pattern(SIZES[struct_of(k)], fid + 3 * i)
            elif k == "I":
                data = struct.pack("<3i", -5 - i, 70000 + i, 11)
            else:
                data = struct.pack("<3Q", 0x5B00000100 + i, 0x5B00000200, 0x5B00000300)
            blobs.append(f"blob {nb} {data.hex()}")
            slots.append(f"@{nb}")
            want.append(data)
            nb += 1
            continue
        slots.append(v)
        want.append(v & 0xFFFFFFFF if k == "f" else v)
    return slots, blobs, want


SIZES = {}                                         # sizeof the parameter structs, as the harness printed them (set by `table`)


def test_each_stub_sees_each_argument_in_its_position_with_the_headers_type_and_the_slots_value(harness, table):
    script, expect = [], []
    for fid, _, name in FNS:
        slots, blobs, want = slot_values(fid, table["kinds"][fid][1])
        script += blobs + [op_line(fid, slots), "create", f"launch {STREAM:x}"]
        expect.append((fid, name, want))
    out = harness.run(script)
    assert [w for w in out if w[0] in ("create", "launch")] == [["create", "0", "1"], ["launch", "0", "-1"]] * len(FNS)
    calls = calls_of(out)
    assert [c["name"] for c in calls] == [name for _, name, _ in expect]
    for call, (fid, name, want) in zip(calls, expect):
        params, kinds = params_of(name), table["kinds"][fid][1]
        assert len(call["args"]) == len(params), name
        structs, ints, ptrs = [], [], []
        for i, ((cls, image), (ctype, pname)) in enumerate(zip(call["args"], params)):
            where = f"{name} slot {i} ({ctype} {pname})"
            assert cls == S.type_class(ctype), where
            if i == len(params) - 1:
                assert image == STREAM, f"{name}: the stream was not handed through"
            elif isinstance(want[i], bytes):
                assert image != 0, where
                {"G": structs, "A": structs, "I": ints, "Q": ptrs}[kinds[i]].append(want[i])
            else:
                assert image == want[i], f"{where}: the stub saw {image:#x}, the slot holds {want[i]:#x}"
        assert call["structs"] == structs, f"{name}: parameter structs"
        assert call["ints"] == [v for b in ints for v in struct.unpack("<3i", b)], f"{name}: host int array"
        assert call["ptrs"] == [v for b in ptrs for v in struct.unpack("<3Q", b)], f"{name}: host pointer array"


# ---- 2. a failing op in a multi-op plan ------------------------------------------------------------------------------------------
def test_launch_stops_at_the_failing_op_and_reports_it(harness, table):
    by_name = {name: fid for fid, _, name in FNS}
    three = [by_name[n] for n in ("da_mul_scalar", "da_transpose_bf16", "da_advance_step")]
    script = []
    for fid in three:
        slots, blobs, _ = slot_values(fid, table["kinds"][fid][1])
        script += blobs + [op_line(fid, slots)]
    script += ["create", f"status {three[1]} {UNSUPPORTED}", f"launch {STREAM:x}", f"status {three[1]} 0", f"launch {STREAM:x}"]
    out = harness.run(script)
    assert out[0] == ["create", "0", "3"]
    first = out[1:out.index(["launch", "0", "-1"])]
    assert first[0] == ["launch", str(UNSUPPORTED), "1"]
    assert [c["name"] for c in calls_of(first)] == ["da_mul_scalar", "da_transpose_bf16"]          # op 2 was not called
    rest = out[out.index(["launch", "0", "-1"]):]
    assert [c["name"] for c in calls_of(rest)] == ["da_mul_scalar", "da_transpose_bf16", "da_advance_step"]


# ---- 3. deep copies ----------------------------------------------------------------------------------------------------------------
def rope_op(fid, kinds, parts, col_blob, wt_blob):
    slots = []
    for i, k in enumerate(kinds):
        slots.append({"n": u64(parts), "I": col_blob, "Q": wt_blob, "p": 0x5A00000000 + 16 * i, "f": f32_bits(1.5)}.get(k, 7 + i))
    return op_line(fid, slots)


def test_plan_keeps_its_own_copies_of_structs_and_host_arrays(harness, table):
    by_name = {name: fid for fid, _, name in FNS}
    g0, g1, g2 = (pattern(SIZES["da_gemm_params"], s) for s in (1, 2, 3))
    a0 = pattern(SIZES["da_attention_params"], 4)
    col, wts = struct.pack("<3i", 0, 64, -9), struct.pack("<3Q", 0x5B00000100, 0, 0x5B00000300)
    rope = by_name["da_rmsnorm_rope_bf16"]
    script = [f"blob {i} {b.hex()}" for i, b in enumerate((g0, g1, g2, a0, col, wts))]
    script += [f"op {by_name['da_gemm_bf16']} @0", f"op {by_name['da_gemm_pair_bf16']} @1 @2", f"op {by_name['da_attention_bf16']} @3",
               rope_op(rope, table["kinds"][rope][1], 3, "@4", "@5"), "create", "mutate", f"launch {STREAM:x}"]
    out = harness.run(script)
    assert out[:2] == [["create", "0", "4"], ["launch", "0", "-1"]]
    calls = calls_of(out)
    assert [c["structs"] for c in calls] == [[g0], [g1, g2], [a0], []]
    assert calls[3]["ints"] == [0, 64, -9] and calls[3]["ptrs"] == [0x5B00000100, 0, 0x5B00000300]


@pytest.mark.parametrize("parts", [0, 1, 64])
def test_host_arrays_of_every_admissible_length_are_copied(harness, table, parts):
    rope = {name: fid for fid, _, name in FNS}["da_rmsnorm_rope_bf16"]
    ints = [(-1) ** j * (j + 1) for j in range(parts)]
    ptrs = [0x5B00000000 + 8 * j for j in range(parts)]
    script = [f"blob 0 {struct.pack(f'<{parts}i', *ints).hex() or '-'}", f"blob 1 {struct.pack(f'<{parts}Q', *ptrs).hex() or '-'}",
              rope_op(rope, table["kinds"][rope][1], parts, "@0", "@1"), "create", "mutate", f"launch {STREAM:x}"]
    if parts == 0:                                                           # NULL arrays are fine when there is nothing in them
        script += [rope_op(rope, table["kinds"][rope][1], 0, 0, 0), "create", f"launch {STREAM:x}"]
    out = harness.run(script)
    assert [w for w in out if w[0] != "call"] == [["create", "0", "1"], ["launch", "0", "-1"]] * (2 if parts == 0 else 1)
    for call in calls_of(out):
        assert call["ints"] == ints and call["ptrs"] == ptrs
        assert call["args"][table["kinds"][rope][1].index("n")] == ("i", parts)


@pytest.mark.parametrize("parts", [65, -1, -(1 << 31)])
def test_host_arrays_longer_than_64_or_negative_are_refused(harness, table, parts):
    rope = {name: fid for fid, _, name in FNS}["da_rmsnorm_rope_bf16"]
    script = [f"blob 0 {bytes(4 * 65).hex()}", f"blob 1 {bytes(8 * 65).hex()}", rope_op(rope, table["kinds"][rope][1], parts, "@0", "@1"),
              "create", f"launch {STREAM:x}"]
    out = harness.run(script)
    assert out == [["create", str(INVALID), "-1"], ["launch", str(INVALID), "-1"]]


# ---- 4. relocation completeness -----------------------------------------------------------------------------------------------------
def struct_image(struct_name, table, pointers):
    """The bytes of a parameter struct whose every 8-byte word outside the pointer fields LOOKS like an address inside R0 (a
    relocated workspace_bytes / ld_vt would show), with the given {field: address} pointers and NULL in the others."""
    n = SIZES[struct_name]
    raw = bytearray(b"".join(struct.pack("<Q", R0[0] + 0x100 + 8 * k) for k in range((n + 7) // 8))[:n])
    for name, off, size, is_ptr in table["fields"][struct_name]:
        if is_ptr:
            assert size == 8
            raw[off:off + 8] = struct.pack("<Q", pointers.get(name, 0))
    return bytes(raw)


def expect_struct(struct_name, table, raw):
    out = bytearray(raw)
    for name, off, size, is_ptr in table["fields"][struct_name]:
        if is_ptr:
            out[off:off + 8] = struct.pack("<Q", moved(struct.unpack_from("<Q", raw, off)[0]))
    return bytes(out)


def test_pointer_fields_come_from_the_header_and_match_the_ctypes_mirrors(table):
    from diffusers_amd import _lib as L
    for struct_name, mirror in (("da_gemm_params", L.GemmParams), ("da_attention_params", L.AttentionParams)):
        from_header = S.pointer_fields(DOC, struct_name)
        assert from_header == [n for n, _, _, p in table["fields"][struct_name] if p]
        assert from_header == [n for n, t in mirror._fields_ if t is C.c_void_p]
        assert [(n, o, s) for n, o, s, _ in table["fields"][struct_name]] == [(n, getattr(mirror, n).offset, getattr(mirror, n).size)
                                                                               for n, _ in mirror._fields_]
        assert SIZES[struct_name] == C.sizeof(mirror)
    assert len(S.pointer_fields(DOC, "da_gemm_params")) == 19 and len(S.pointer_fields(DOC, "da_attention_params")) == 6


@pytest.mark.parametrize("letter", ["G", "A"])
def test_every_pointer_field_of_the_parameter_structs_is_relocated_and_nothing_else(harness, table, letter):
    struct_name = struct_of(letter)
    fid = {name: fid for fid, _, name in FNS}["da_gemm_bf16" if letter == "G" else "da_attention_bf16"]
    fields = S.pointer_fields(DOC, struct_name)
    # one plan per field (the others NULL), then all of them at once
    cases = [{f: R1[0] + 0x40 + 8 * i} for i, f in enumerate(fields)]
    cases.append({f: (R1[0] + 0x40 + 8 * i) if i % 2 else (R0[0] + 0x9000 + 8 * i) for i, f in enumerate(fields)})
    script, raws = [], []
    for i, ptrs in enumerate(cases):
        raws.append(struct_image(struct_name, table, ptrs))
        script += [f"blob {i} {raws[-1].hex()}", f"op {fid} @{i}", "create", "relocate", REGIONS, f"launch {STREAM:x}"]
    out = harness.run(script)
    assert len(out) == 5 * len(cases)
    for i, (ptrs, raw) in enumerate(zip(cases, raws)):
        create, count, reloc, launch, call = out[5 * i:5 * i + 5]
        what = f"{struct_name}.{'/'.join(ptrs) if len(ptrs) == 1 else '(all)'}"
        assert create == ["create", "0", "1"] and launch == ["launch", "0", "-1"]
        assert count == ["relocate", "0", str(len(ptrs))], f"{what}: with no region every non-NULL address is unmatched"
        assert reloc == ["relocate", "0", "0"], f"{what}: an address inside a region was not visited"
        got = S.parse_call(call)["structs"][0]
        want = expect_struct(struct_name, table, raw)
        for name, off, size, is_ptr in table["fields"][struct_name]:
            assert got[off:off + size] == want[off:off + size], f"{struct_name}.{name} after relocating {what}"
        assert got == want, f"{what}: padding bytes changed"


def test_every_pointer_slot_and_every_pointer_array_entry_is_relocated_and_nothing_else(harness, table):
    script, expect = [], []
    for fid, _, name in FNS:
        kinds = table["kinds"][fid][1]
        slots, want, nb, n_ptr = [], [], 0, 0
        for i, k in enumerate(kinds):
            if k == "p":
                v = (R1[0] + 0x80 + 8 * i) if i % 2 else (R0[0] + 0xF000 + 8 * i)
                n_ptr += 1
            elif k == "l":
                v = R0[0] + 0x800 + i                                       # a long long that looks like an address in a region
            elif k == "i":
                v = u64(-3 - i)
            elif k == "f":
                v = f32_bits(i + 0.37)
            elif k == "n":
                v = 3
            else:
                if k in "GA":
                    fields = S.pointer_fields(DOC, struct_of(k))
                    data = struct_image(struct_of(k), table, {f: R1[0] + 0x100 + 8 * (j + i) for j, f in enumerate(fields)})
                    n_ptr += len(fields)
                elif k == "I":
                    data = struct.pack("<3i", 1, 2, 3)
                else:
                    data = struct.pack("<3Q", R1[0] + 0x300, 0, R0[0] + 0x308)   # a NULL entry stays NULL and is not counted
                    n_ptr += 2
                script.append(f"blob {nb} {data.hex()}")
                slots.append(f"@{nb}")
                want.append(data)
                nb += 1
                continue
            slots.append(v)
            want.append(v)
        script += [op_line(fid, slots), "create", "relocate", REGIONS, f"launch {STREAM:x}"]
        expect.append((name, kinds, want, n_ptr))
    out = harness.run(script)
    assert len(out) == 5 * len(FNS)
    for j, (name, kinds, want, n_ptr) in enumerate(expect):
        create, count, reloc, launch, call = out[5 * j:5 * j + 5]
        assert create == ["create", "0", "1"] and launch == ["launch", "0", "-1"], name
        assert count == ["relocate", "0", str(n_ptr)], f"{name}: {n_ptr} non-NULL device addresses, the plan visited {count[2]}"
        assert reloc == ["relocate", "0", "0"], name
        call = S.parse_call(call)
        structs, ptrs = [], []
        for i, (k, (cls, image)) in enumerate(zip(kinds, call["args"])):
            where = f"{name} slot {i} ({' '.join(params_of(name)[i])})"
            if k in "GA":
                structs.append(expect_struct(struct_of(k), table, want[i]))
            elif k == "Q":
                ptrs += [moved(v) for v in struct.unpack("<3Q", want[i])]
            elif k == "p":
                assert image == moved(want[i]) != want[i], f"{where}: {want[i]:#x} -> {image:#x}, expected {moved(want[i]):#x}"
            elif k != "I":
                assert image == want[i], f"{where}: not a device address, but {want[i]:#x} became {image:#x}"
        assert call["structs"] == structs and call["ptrs"] == ptrs, name
        assert call["args"][-1] == ("p", STREAM), name


def test_region_edges_null_and_unmatched_count(harness, table):
    """One address per edge in a pointer slot, a struct field and a pointer array entry: the last byte of a region moves, base + bytes
    does not, NULL stays NULL and is not counted, `unmatched` counts exactly the addresses outside every region."""
    by_name = {name: fid for fid, _, name in FNS}
    edges = [R1[0] + R1[1] - 1, R1[0] + R1[1], 0, R1[0] - 1, R1[0], R0[0] + R0[1] - 1, R0[0] + R0[1]]
    outside = sum(1 for v in edges if v and moved(v) == v)
    assert outside == 3
    script = []
    # p slots: da_groupnorm_nhwc_bf16 has seven
    gn = by_name["da_groupnorm_nhwc_bf16"]
    kinds = table["kinds"][gn][1]
    p_slots = [i for i, k in enumerate(kinds) if k == "p"]
    assert len(p_slots) >= len(edges)
    slots = [0] * len(kinds)
    for i, v in zip(p_slots, edges):
        slots[i] = v
    script += [op_line(gn, slots), "create", REGIONS, f"launch {STREAM:x}"]
    # struct fields
    fields = S.pointer_fields(DOC, "da_gemm_params")
    raw = struct_image("da_gemm_params", table, dict(zip(fields, edges)))
    script += [f"blob 0 {raw.hex()}", f"op {by_name['da_gemm_bf16']} @0", "create", REGIONS, f"launch {STREAM:x}"]
    # Q entries
    rope = by_name["da_rmsnorm_rope_bf16"]
    n = len(edges)
    script += [f"blob 1 {bytes(4 * n).hex()}", f"blob 2 {struct.pack(f'<{n}Q', *edges).hex()}"]
    script.append(op_line(rope, [{"n": n, "I": "@1", "Q": "@2"}.get(k, 0) for k in table["kinds"][rope][1]]))
    script += ["create", REGIONS, f"launch {STREAM:x}"]
    out = harness.run(script)
    assert [w for w in out if w[0] != "call"] == [["create", "0", "1"], ["relocate", "0", str(outside)], ["launch", "0", "-1"]] * 3
    calls = calls_of(out)
    assert [calls[0]["args"][i][1] for i in p_slots[:n]] == [moved(v) for v in edges]
    assert calls[1]["structs"] == [expect_struct("da_gemm_params", table, raw)]
    assert calls[2]["ptrs"] == [moved(v) for v in edges]
    assert [moved(v) == v for v in edges] == [False, True, True, True, False, False, True]


# ---- the recorder: launches a plan cannot replay -------------------------------------------------------------------------------------
def test_every_launch_entry_point_of_the_header_is_planned_reported_or_passed_through_by_design():
    from diffusers_amd import _lib as L
    launches = {name for name, (_, params) in DOC["protos"].items() if ("void*", "stream") in params}
    assert launches >= set(L.FN_IDS) and len(launches) > len(L.FN_IDS)
    sets = (set(L.FN_IDS), set(L.NOT_PLANNABLE), set(L.PASS_THROUGH))
    assert set().union(*sets) == launches, "a launch entry point is in none of FN_IDS / NOT_PLANNABLE / PASS_THROUGH (or a name there is no launch)"
    assert sum(len(s) for s in sets) == len(launches), "an entry point is in more than one of the three"
    assert set(L.NOT_PLANNABLE) == {"da_vae_conv_in_image", "da_vae_posterior_latents", "da_flux_prepare_latents"}
    assert all(isinstance(why, str) and why.strip() for why in L.PASS_THROUGH.values())
    assert {name for _, _, name in FNS} == set(L.FN_IDS)


class _FakeLib:
    """Stands in for the ctypes library behind plan._Proxy: every entry point returns `status` and counts its calls."""

    def __init__(self, status):
        self.status, self.called = status, []

    def __getattr__(self, name):
        if not name.startswith("da_"):
            raise AttributeError(name)

        def fn(*args):
            self.called.append(name)
            return self.status
        return fn


@pytest.mark.parametrize("name", ["da_vae_conv_in_image", "da_vae_posterior_latents", "da_flux_prepare_latents"])
def test_a_launch_the_plan_cannot_replay_is_executed_and_noted_as_foreign(name):
    from diffusers_amd import _lib as L, plan as P
    args = [0] * len(L.SIGNATURES[name][1])
    rec = P.Recorder()
    ok = _FakeLib(L.DA_OK)
    assert getattr(P._Proxy(ok, rec), name)(*args) == L.DA_OK
    assert ok.called == [name] and rec.foreign == [name] and rec.ops == [] and rec.names == []
    rec = P.Recorder()                                      # a refused call launched nothing: not part of the step, nothing to report
    refused = _FakeLib(UNSUPPORTED)
    assert getattr(P._Proxy(refused, rec), name)(*args) == UNSUPPORTED
    assert refused.called == [name] and rec.foreign == [] and rec.ops == []


def test_pass_through_and_planned_entry_points_behave_as_before():
    from diffusers_amd import _lib as L, plan as P
    rec = P.Recorder()
    lib = _FakeLib(L.DA_OK)
    proxy = P._Proxy(lib, rec)
    for name in L.PASS_THROUGH:
        assert getattr(proxy, name)(*[0] * len(L.SIGNATURES[name][1])) == L.DA_OK
    assert rec.foreign == [] and rec.ops == [] and lib.called == list(L.PASS_THROUGH)
    assert proxy.da_mul_scalar(0x2000, None, -1.5, -1, 1 << 40, 1, 0x77) == L.DA_OK
    assert rec.names == ["da_mul_scalar"] and rec.foreign == [] and rec.streams == {0x77}
    rec2 = P.Recorder()
    assert P._Proxy(_FakeLib(UNSUPPORTED), rec2).da_mul_scalar(0x2000, None, -1.5, -1, 1 << 40, 1, 0x77) == UNSUPPORTED
    assert rec2.names == [] and rec2.foreign == []


def test_strict_recording_raises_on_a_launch_the_plan_cannot_replay():
    from diffusers_amd import plan as P
    with pytest.raises(RuntimeError, match="da_flux_prepare_latents"):
        with P.recording(strict=True, private_pool=False) as rec:
            rec.foreign.append("da_flux_prepare_latents")          # what the proxy does on a successful call
    with P.recording(strict=False, private_pool=False) as rec:
        rec.foreign.append("da_flux_prepare_latents")
    assert rec.foreign == ["da_flux_prepare_latents"]


def test_device_pointers_of_a_plan_with_host_pointer_arrays():
    """Plan.device_pointers() (what Plan.save() builds its regions from) takes ONE host object per I / Q argument: with a pointer
    array of two entries it used to take one per entry -- the next op's struct, or StopIteration at the end of the list (found by
    tests/test_plan_entry_points_gpu.py::rmsnorm_rope, the first plan with such an array that was ever saved)."""
    from diffusers_amd import _lib as L, plan as P
    rec = P.Recorder()
    col, wts = (C.c_int * 2)(0, 128), (C.c_void_p * 2)(0x20040, 0x20080)
    rec.note("da_rmsnorm_rope_bf16", L.FN_IDS["da_rmsnorm_rope_bf16"],
             (0x10020, 384, 64, 64, 2, 64, 2, col, wts, 1e-6, 0x200c0, 0x20100, 16, 1, 0x77))
    g = L.GemmParams()
    g.A, g.W, g.C = 0x30000, 0x30100, 0x30200
    rec.note("da_gemm_bf16", L.FN_IDS["da_gemm_bf16"], (C.byref(g), 0x77))
    pl = P.Plan(rec)
    assert pl.device_pointers() == [0x10020, 0x20040, 0x20080, 0x200c0, 0x20100, 0x30000, 0x30100, 0x30200]
    pl.close()
