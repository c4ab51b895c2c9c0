"""The whole ctypes mirror (signalalign_amd/_capi.py) held against the C headers, without a device: every registered struct's size and
field offsets against a C program compiled from the headers; every struct of the public header either mirrored or named here as
not mirrored; every bound function's restype and argtypes against its prototype, kind by kind.  The comparison functions are
themselves run on a deliberately wrong mirror."""
import ctypes as C
import os
import subprocess

import numpy as np

from signalalign_amd import _capi

import abi_header as hdr

# structs of the public header that Python reads without a mirror of their own, and how
NOT_MIRRORED = {
    "sa_pair16_t": "read in place as a uint64 array [n, 2] (Batch.pairs16, Batch.results_view)",
    "sa_ea_pair_t": "copied out as an int32 array [n, 2] (event_align_batch, raw_event_align_batch)",
    "sa_mea_pair_t": "copied out as an int32 array [n, 2] (mea_batch, Batch.mea)",
    "sa_assignment_t": "copied out as an int64 array [n, 2] (expect_batch)",
    "sa_noise_scale_t": "passed as a float64 array [n, 2] (Batch(noise=...))",
}


def derived_dtypes():
    """{C type: X_DTYPE} for the module's dtypes that are a second form of a registered structure (X_DTYPE of class X); every other
    X_DTYPE of the module must be a registered mirror itself"""
    out = {}
    for name in dir(_capi):
        if name.endswith("_DTYPE") and not any(getattr(_capi, name) is m for m in _capi.ABI.values()):
            struct = getattr(_capi, "".join(w.capitalize() for w in name[:-len("_DTYPE")].split("_")))
            assert _capi.ABI[struct._c_name_] is struct, name
            out[struct._c_name_] = getattr(_capi, name)
    return out


def mirror_fields(mirror, dtype=None):
    """(size, {field: offset}) per form of the mirror: the C.Structure or registered np.dtype, and the dtype derived from a structure"""
    forms = []
    for m in (mirror, dtype):
        if isinstance(m, np.dtype):
            forms.append((m.itemsize, {n: m.fields[n][1] for n in m.names}))
        elif m is not None:
            forms.append((C.sizeof(m), {n: getattr(m, n).offset for n, _ in m._fields_}))
    return forms


def layout_program(registry, headers):
    lines = ["#include <stddef.h>", "#include <stdio.h>"] + ['#include "%s"' % os.path.basename(h) for h in headers]
    lines.append("int main(void) {")
    for c_name, mirror in registry.items():
        lines.append('    printf("%s  %%zu\\n", sizeof(%s));' % (c_name, c_name))
        for field in mirror_fields(mirror)[0][1]:
            lines.append('    printf("%s %s %%zu\\n", offsetof(%s, %s));' % (c_name, field, c_name, field))
    return "\n".join(lines + ["    return 0;", "}", ""])


def c_layouts(registry, tmp_path):
    """{(C type, field or ""): offset or size} as the C compiler lays the registry's types out"""
    src, exe = tmp_path / "abi_layout.c", tmp_path / "abi_layout"
    src.write_text(layout_program(registry, [hdr.PUBLIC_HEADER, hdr.IO_HEADER]))
    cc = os.environ.get("CC", "cc")
    subprocess.run([cc, "-std=c11"] + ["-I" + d for d in hdr.INCLUDE_DIRS] + ["-o", str(exe), str(src)], check=True, timeout=120)
    out = subprocess.run([str(exe)], check=True, capture_output=True, text=True, timeout=60).stdout
    return {(t, f): int(v) for t, f, v in (line.split(" ") for line in out.splitlines())}


def layout_differences(registry, layouts, dtypes):
    """[(C type, field or "", what C says, what the mirror says)] and the number of comparisons made"""
    bad, n = [], 0
    for c_name, mirror in registry.items():
        for size, offsets in mirror_fields(mirror, dtypes.get(c_name)):
            for field, got in [("", size)] + list(offsets.items()):
                n += 1
                if layouts[(c_name, field)] != got:
                    bad.append((c_name, field, layouts[(c_name, field)], got))
    return bad, n


def signature_differences(table, protos):
    """[(function, position or "return" or "count", the header's kind, the table's kind)]; a kind neither side could reduce (None) is
    a difference too"""
    bad = []
    for name, (restype, argtypes) in table.items():
        if name not in protos:
            bad.append((name, "prototype", None, None))
            continue
        (c_ret, c_args), (p_ret, p_args) = protos[name], hdr.signature_kinds(restype, argtypes)
        if c_ret != p_ret or c_ret is None:
            bad.append((name, "return", c_ret, p_ret))
        if len(c_args) != len(p_args):
            bad.append((name, "count", len(c_args), len(p_args)))
        bad += [(name, i, c, p) for i, (c, p) in enumerate(zip(c_args, p_args)) if c != p or c is None]
    return bad


def test_every_registered_struct_is_laid_out_as_c_lays_it_out(tmp_path):
    registry, dtypes = dict(_capi.ABI), derived_dtypes()
    assert len(dtypes) == 7
    layouts = c_layouts(registry, tmp_path)
    bad, n = layout_differences(registry, layouts, dtypes)
    assert bad == []
    n_fields = sum(len(mirror_fields(m)[0][1]) for m in registry.values())
    print("%d structs, %d fields, %d comparisons" % (len(registry), n_fields, n))
    assert len(layouts) == len(registry) + n_fields
    assert n == len(layouts) + sum(1 + len(d.names) for d in dtypes.values())
    # the sizes the header's comments promise are what both sides have
    assert layouts[("sa_train_job_map_t", "")] == 24 and layouts[("sa_pair_t", "")] == 24

    # the checker is itself checked on a deliberately wrong mirror -- x_sign and site_strand change places: it reports exactly those
    # two, in the structure and in the dtype derived from it
    class SwappedTrainJobMap(C.Structure):
        _fields_ = [("contig", C.c_int32), ("site_strand", C.c_int32), ("x0", C.c_int64), ("x_sign", C.c_int32), ("pad", C.c_int32)]
    assert sorted(n for n, _ in SwappedTrainJobMap._fields_) == sorted(n for n, _ in _capi.TrainJobMap._fields_)
    assert C.sizeof(SwappedTrainJobMap) == 24
    wrong, _ = layout_differences({"sa_train_job_map_t": SwappedTrainJobMap}, layouts,
                                  {"sa_train_job_map_t": np.dtype(SwappedTrainJobMap)})
    assert wrong == [("sa_train_job_map_t", "site_strand", 16, 4), ("sa_train_job_map_t", "x_sign", 4, 16)] * 2


def test_both_forms_of_a_struct_are_one_declaration():
    for name in ("SITE_CALL", "POSITION_CALL", "TRUTH_SITE", "TRAIN_SITE", "TRAIN_JOB_MAP", "SNP_SITE", "PAIR"):
        struct = getattr(_capi, "".join(w.capitalize() for w in name.split("_")))
        assert getattr(_capi, name + "_DTYPE") == np.dtype(struct), name
    for c_name, mirror in _capi.ABI.items():
        assert isinstance(mirror, np.dtype) or mirror._c_name_ == c_name


def test_every_struct_of_the_header_is_mirrored_or_named_as_not():
    in_header = hdr.struct_names(hdr.header_text())
    assert len(in_header) == len(set(in_header))
    from_io = {c for c, m in _capi.ABI.items() if not isinstance(m, np.dtype) and m._c_header_.endswith("sa_io.h")}
    assert from_io == {"sa_cigar_t", "sa_rawread_t"} and from_io <= set(hdr.struct_names(hdr.header_text(hdr.IO_HEADER)))
    mirrored = set(_capi.ABI) - from_io
    assert not mirrored & set(NOT_MIRRORED)
    assert mirrored | set(NOT_MIRRORED) == set(in_header), (mirrored | set(NOT_MIRRORED)) ^ set(in_header)


def test_every_bound_function_is_declared_as_its_prototype():
    public, io = hdr.prototypes(hdr.header_text()), hdr.prototypes(hdr.header_text(hdr.IO_HEADER))
    assert set(public) == set(_capi.SIGNATURES) == set(_capi.EXPORTS)          # no export lacks a table entry
    assert set(_capi.IO_SIGNATURES) <= set(io) and not set(_capi.IO_SIGNATURES) & set(public)
    unknown = [(n, r, a) for n, (r, a) in list(public.items()) + list(io.items()) if r is None or None in a]
    assert unknown == []
    assert signature_differences(_capi.SIGNATURES, public) == []
    assert signature_differences(_capi.IO_SIGNATURES, io) == []
    n_void = sum(1 for r, _ in _capi.SIGNATURES.values() if r is None)
    print("%d + %d prototypes, %d parameters, %d void" % (len(public), len(_capi.IO_SIGNATURES),
                                                          sum(len(a) for _, a in _capi.SIGNATURES.values()), n_void))
    # what lib() set on the loaded library is the table
    L = _capi.lib()
    for name, (restype, argtypes) in list(_capi.SIGNATURES.items()) + list(_capi.IO_SIGNATURES.items()):
        fn = getattr(L, name)
        assert fn.restype is restype and list(fn.argtypes) == list(argtypes), name
    # the checker is itself checked: one int64_t narrowed to 32 bits is reported, and only that
    restype, argtypes = _capi.SIGNATURES["sa_batch_pairs"]
    assert [hdr.ctypes_kind(a) for a in argtypes] == ["ptr", "i64", "ptr", "i64"]
    narrowed = {"sa_batch_pairs": (restype, argtypes[:3] + [C.c_int32])}
    assert signature_differences(narrowed, public) == [("sa_batch_pairs", 3, "i64", "i32")]
    assert signature_differences({"sa_batch_pairs": (None, argtypes[:3])}, public) == [
        ("sa_batch_pairs", "return", "i32", "void"), ("sa_batch_pairs", "count", 4, 3)]
    assert hdr.c_kind("long double x") is None and hdr.ctypes_kind(C.c_float) is None
