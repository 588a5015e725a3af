"""The C-ABI library loads without a GPU, exports every symbol include/gaml_hip.h declares, and
refuses to score without a device (there is no CPU scoring path in the product)."""
import ctypes
import os
import re

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def declared_symbols(header="gaml_hip.h"):
    text = open(os.path.join(ROOT, "include", header)).read()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    return sorted(set(re.findall(r"\b(gaml_hip_[a-z_0-9]+)\s*\(", text)))


def test_every_declared_symbol_is_exported(built):
    """The product library exports exactly the drop-in surface (include/gaml_hip.h) and NOTHING of the test / tuning
    surface (include/gaml_hip_debug.h: entry points, A/B knobs, in-kernel time stamps); the development build, the same
    sources with -DGAML_HIP_DEV, exports both."""
    import subprocess
    names = declared_symbols()
    assert len(names) >= 30
    assert not [n for n in names if "_debug_" in n]  # the drop-in header carries no debug surface
    dbg = declared_symbols("gaml_hip_debug.h")
    assert len(dbg) >= 10 and all("_debug_" in n for n in dbg)
    exported = {}
    for lib in ("libgaml_hip.so", "libgaml_hip_dev.so"):
        out = subprocess.check_output(["nm", "-D", "--defined-only", os.path.join(ROOT, "gaml_amd", lib)], text=True)
        exported[lib] = {ln.split()[-1] for ln in out.splitlines() if ln.split()}
    release, dev = exported["libgaml_hip.so"], exported["libgaml_hip_dev.so"]
    assert not [n for n in names if n not in release], [n for n in names if n not in release]
    assert not [n for n in names + dbg if n not in dev], [n for n in names + dbg if n not in dev]
    assert not [n for n in release if "debug" in n], [n for n in release if "debug" in n]
    # ... and no kernel instantiation with in-kernel time stamps (paired_score_kernel<false, true>: GEN, TL, COV) in the product
    blob = open(os.path.join(ROOT, "gaml_amd", "libgaml_hip.so"), "rb").read()
    assert b"paired_score_kernelILb0ELb1ELb0E" not in blob
    assert b"paired_score_kernelILb0ELb1ELb0E" in open(os.path.join(ROOT, "gaml_amd", "libgaml_hip_dev.so"), "rb").read()
    lib = ctypes.CDLL(os.path.join(ROOT, "gaml_amd", "libgaml_hip.so"))
    assert not [n for n in names if not hasattr(lib, n)]


def test_library_was_built_from_this_tree(built):
    """gaml_hip_version() carries the hash of the sources the .so was built from (csrc/Makefile: SRC_HASH): the GPU box
    receives the prebuilt library, this is how a stale one is noticed."""
    import hashlib
    import subprocess
    from gaml_amd import api
    # the ONE list of sources: the Makefile's (everything in csrc/ and include/, so a new header cannot be left out)
    rel = subprocess.check_output(["make", "-s", "-C", os.path.join(ROOT, "gaml_amd", "csrc"), "print-srcs"], text=True).split()
    assert "gaml_amd/csrc/pacbio_sweep.hip.h" in rel and "include/gaml_hip_debug.h" in rel and len(rel) >= 14
    h = hashlib.sha256()
    for r in rel:
        h.update(open(os.path.join(ROOT, r), "rb").read())
    assert api.version().endswith("src " + h.hexdigest()[:16]), api.version()
    assert " dev " in api.version()  # tests load the development build (tests/conftest.py)
    rel = ctypes.CDLL(os.path.join(ROOT, "gaml_amd", "libgaml_hip.so"))
    rel.gaml_hip_version.restype = ctypes.c_char_p
    v = rel.gaml_hip_version().decode()
    assert v.endswith("src " + h.hexdigest()[:16]) and " dev " not in v, v


def test_record_layouts_match_the_reference_structs(built):
    from gaml_amd import api
    assert api.ALIGMENT.itemsize == 16        # Aligment = 4 x int32 (graph.h:211-231)
    assert api.PACBIO_ALIGMENT.itemsize == 24  # PacbioAligment = 3 x int32 + logdouble (graph.h:516-535)
    assert ctypes.sizeof(api.PairedCfg) == 64 and ctypes.sizeof(api.SingleCfg) == 48


def test_host_only_context_refuses_to_score(built):
    from gaml_amd import api, synth
    genome = synth.make_genome(5000, 1)
    g = synth.make_graph(genome, synth.cut_lengths(5000, 1, long_rng=(900, 1500)))
    pr = synth.make_paired_reads(genome, 50, 100, 250.0, 25.0, 0.01, 1)
    ctx = api.Context(device=-1)
    ctx.set_graph(*g.packed())
    rs = ctx.add_paired(api.paired_cfg(250.0, 25.0), *synth.pack_reads(pr.mate1), *synth.pack_reads(pr.mate2))
    assert ctx.num_readsets() == 1 and ctx.readset_reads(rs) == 50 and ctx.readset_kind(rs) == 1
    assert ctx.num_nodes() == g.n_nodes and ctx.node_len(0) == g.node_len(0)
    with pytest.raises(api.GamlHipError) as e:
        ctx.calc_prob([synth.genome_walk(g)])
    assert e.value.code == api.ENODEVICE
    with pytest.raises(api.GamlHipError):
        ctx.calc_partials([synth.genome_walk(g)])
    with pytest.raises(api.GamlHipError):
        ctx.read_probs(rs)


def test_argument_errors(built):
    from gaml_amd import api
    ctx = api.Context(device=-1)
    with pytest.raises(api.GamlHipError):  # odd node count: twin of i is i^1
        ctx.set_graph(np.frombuffer(b"ACGT", np.uint8), np.array([0, 2, 3, 4], np.int64))
    with pytest.raises(api.GamlHipError):
        ctx.load_graph("/nonexistent/LastGraph")
    with pytest.raises(api.GamlHipError):
        ctx.add_paired_fastq(api.paired_cfg(300, 30), "/nonexistent/a.fq", "/nonexistent/b.fq")
    with pytest.raises(api.GamlHipError):  # device ordinal that does not exist
        api.Context(device=4096)
    assert "gaml_hip" in api.version()


def declared_enums(header="gaml_hip_debug.h"):
    """{enum name: {enumerator: number}} of a header whose enumerators all carry an explicit number"""
    text = open(os.path.join(ROOT, "include", header)).read()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    enums = {}
    for name, body in re.findall(r"\benum\s+(gaml_hip_[a-z_]+)\s*\{(.*?)\}", text, flags=re.S):
        entries = [e.strip() for e in body.split(",") if e.strip()]
        assert all(re.fullmatch(r"GAML_HIP_[A-Z0-9_]+\s*=\s*\d+", e) for e in entries), (name, entries)
        enums[name] = {e.split("=")[0].strip(): int(e.split("=")[1]) for e in entries}
    return enums


# what the numbers 0-24 meant when the knobs got their names: libraries built from older trees are addressed by these numbers
KNOBS_0_TO_24 = ["GRID_CAP_COMPACT", "SCORE_LDS_BYTES", "FINISH_MODE", "TIMELINE", "NO_MEMO", "ALIGNER_ROUTE", "DELTA_POLICY", "NO_SPIN",
                 "UPLOAD_ROUTE", "ALIGNER_TIMED", "GRID_CAP_CLASS1", "BATCH_ROUTE", "PLAN_WHOLE_SET", "NO_RESIDENT_TABLES",
                 "REBUILD_ON_CALLER", "NO_RETIRE", "KEEP_DOMINATED", "NO_OCC_DEVICE", "GAP_FALLBACK", "NO_STATIC_INDEX",
                 "GRID_CAP_COMPACT_REST", "NO_COV_INSTANCE", "DELTA_ONE_BLOCK", "ALIGNER_FIRST_CAP", "DELTA_SPILL_CAP"]


def test_knob_registry_matches_the_binding_and_keeps_its_numbers(built):
    """enum gaml_hip_knob (include/gaml_hip_debug.h) is the one list of the development build's knobs: api.Knob repeats it name
    for name, the numbers run from 0 to GAML_HIP_KNOB_COUNT - 1 without a gap, and 0-24 are what they were -- a new knob
    takes a new number. The enums of the knobs' named values are repeated in api as well."""
    from gaml_amd import api
    enums = declared_enums()
    knobs = {n[len("GAML_HIP_KNOB_"):]: v for n, v in enums["gaml_hip_knob"].items()}
    assert len(knobs) == len(enums["gaml_hip_knob"]) and all(n.startswith("GAML_HIP_KNOB_") for n in enums["gaml_hip_knob"])
    count = knobs.pop("COUNT")
    assert {k.name: int(k) for k in api.Knob} == knobs and len(api.Knob.__members__) == len(knobs)  # (no alias either)
    assert sorted(knobs.values()) == list(range(count)) and api.KNOB_COUNT == count
    assert [api.Knob(i).name for i in range(25)] == KNOBS_0_TO_24
    values = {"gaml_hip_aligner_route": ("GAML_HIP_ALIGNER_", api.AlignerRoute),
              "gaml_hip_delta_policy": ("GAML_HIP_DELTA_", api.DeltaPolicy), "gaml_hip_upload_route": ("GAML_HIP_UPLOAD_", api.UploadRoute),
              "gaml_hip_batch_route": ("GAML_HIP_BATCH_", api.BatchRoute)}
    assert set(enums) == set(values) | {"gaml_hip_knob"}
    for name, (prefix, cls) in values.items():
        assert {prefix + v.name: int(v) for v in cls} == enums[name], name


def test_set_knob_checks_its_range(built):
    from gaml_amd import api
    ctx = api.Context(device=-1)
    ctx.debug_set_knob(api.Knob(api.KNOB_COUNT - 1), 0)
    ctx.debug_set_knob(int(api.Knob.NO_MEMO), 0)  # a number still does: what a library built from an older tree is addressed by
    for knob in (api.KNOB_COUNT, -1):
        with pytest.raises(api.GamlHipError) as e:
            ctx.debug_set_knob(knob, 0)
        assert e.value.code == api.EINVAL, knob
