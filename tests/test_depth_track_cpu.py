"""The depth track without a device: the C ABI (header, exports, struct layout in C99), the refusals the host makes before
it looks at the context, the two forms of tests/track_model.py against each other, the run-count bound, write_bedgraph
through profile_from_bedgraph, and the refusals of the file flow."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

import depth_model as dm
import multi_reference as mr
import target_model as tm
import track_model as tk

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("qmcp_hip_depth_track_host", "qmcp_hip_depth_track_device")
PATTERN = 0xA5


def _struct_fields(header, name):
    body = re.search(r"typedef struct %s \{(.*?)\} %s;" % (name, name), header, re.S).group(1)
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    fields = re.findall(r"\b(uint32_t|uint64_t|float)\s+([a-z_, ]+);", body)
    return [(n.strip(), t) for t, group in fields for n in group.split(",")]


def test_header_declares_the_entries_and_the_library_exports_them(pkg):
    with open(os.path.join(ROOT, "include", "qmcp_hip.h")) as f:
        header = f.read()
    for name in NAMES:
        assert re.search(r"\bint\s+" + name + r"\s*\(", header), name
        assert name in pkg.ABI_SYMBOLS
        assert name in pkg.exported_symbols()
    ctype = {"uint32_t": C.c_uint32, "uint64_t": C.c_uint64, "float": C.c_float}
    for struct, mirror in (("qmcp_hip_track_run", pkg.TrackRun), ("qmcp_hip_track_stats", pkg.TrackStats)):
        fields = _struct_fields(header, struct)
        assert [n for n, _ in fields] == [f for f, _ in mirror._fields_], struct
        assert [ctype[t] for _, t in fields] == [t for _, t in mirror._fields_], struct
    assert C.sizeof(pkg.TrackRun) == 24 == pkg.TRACK_RUN_DTYPE.itemsize and C.sizeof(pkg.TrackStats) == 64
    assert pkg.TRACK_RUN_DTYPE.names == tuple(f for f, _ in pkg.TrackRun._fields_) == tk.FIELDS
    assert [pkg.TRACK_RUN_DTYPE.fields[f][1] for f in tk.FIELDS] == [getattr(pkg.TrackRun, f).offset for f in tk.FIELDS]
    for name, value in (("IN", 1), ("KEPT", 2), ("SHORT_ONLY", 4), ("SKIP_ZERO", 8)):
        assert re.search(r"#define QMCP_TRACK_%s %du\b" % (name, value), header) and getattr(pkg, "TRACK_" + name) == value
    assert "n_runs <= min(positions_in_runs, 2 * reads_placed + n_contigs + regions_merged)" in header
    assert pkg.abi_version() == 5 and "#define QMCP_HIP_ABI_VERSION 5" in header


def test_header_is_c99_and_the_struct_sizes_are_24_and_64(pkg, tmp_path):
    head = ("qmcp_hip_ctx*, const uint32_t*, const uint32_t*, const uint32_t*, uint64_t, const uint32_t*, uint32_t, "
            "const uint64_t*, uint32_t, const uint32_t*, const uint32_t*, const uint32_t*, uint32_t, uint32_t, uint32_t, "
            "qmcp_hip_track_run*, uint64_t, uint64_t*, ")
    src = ('#include <stdio.h>\n#include <stddef.h>\n#include "qmcp_hip.h"\nint main(void){\n'
           "int (*h)(" + head + "qmcp_hip_track_stats*) = qmcp_hip_depth_track_host; (void)h;\n"
           "int (*d)(" + head + "void*, qmcp_hip_track_stats*) = qmcp_hip_depth_track_device; (void)d;\n"
           'printf("%zu %zu %zu %zu\\n", sizeof(qmcp_hip_track_run), sizeof(qmcp_hip_track_stats), '
           "offsetof(qmcp_hip_track_run, flags), offsetof(qmcp_hip_track_stats, ms_track));\nreturn 0; }\n")
    exe = tmp_path / "track_abi"
    lib = os.path.join(ROOT, "genome-downsampler_amd", "lib")
    out = subprocess.run(["gcc", "-std=c99", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), "-x", "c", "-",
                          "-L", lib, "-lqmcp_hip", "-Wl,-rpath," + lib, "-o", str(exe)],
                         input=src, text=True, capture_output=True)
    assert out.returncode == 0, out.stderr
    assert subprocess.run([str(exe)], capture_output=True, text=True).stdout.split() == ["24", "64", "20", "60"]


def _call(pkg, flags=3, offs=None, t0=None, t1=None, lengths=(50, 70), columns=True, entry="host"):
    """a track entry on three reads and a null context, every output pre-filled -> (rc, message, untouched)"""
    u32 = lambda a: np.ascontiguousarray(a, np.uint32)
    s, e, ids, lengths = u32([1, 2, 3]), u32([9, 9, 9]), u32([0, 1, 0]), u32(lengths)
    runs = np.full(16 * 24, PATTERN, np.uint8)
    n_runs = np.full(8, PATTERN, np.uint8)
    stats = np.full(C.sizeof(pkg.TrackStats), PATTERN, np.uint8)
    vp = lambda a: a.ctypes.data_as(C.c_void_p)
    p = pkg._p32
    head = (p(s), p(e), p(ids)) if entry == "host" else (vp(s), vp(e), vp(ids))
    if not columns:
        head = (None, head[1], head[2])
    args = [None, *head, 3, p(lengths), lengths.size, None, 5, None if offs is None else p(u32(offs)),
            None if t0 is None else p(u32(t0)), None if t1 is None else p(u32(t1)), 0, flags, 0, vp(runs), 16,
            n_runs.ctypes.data_as(C.POINTER(C.c_uint64))]
    if entry == "device":
        args.append(None)
    fn = pkg._hip.qmcp_hip_depth_track_host if entry == "host" else pkg._hip.qmcp_hip_depth_track_device
    rc = fn(*args, C.cast(vp(stats), C.POINTER(pkg.TrackStats)))
    untouched = all(np.all(a == PATTERN) for a in (runs, n_runs, stats))
    return rc, pkg._hip.qmcp_hip_last_error().decode(), untouched


@pytest.mark.parametrize("entry", ["host", "device"])
def test_refusals_made_on_the_host_need_no_device_and_write_nothing(pkg, entry):
    call = lambda **kw: _call(pkg, entry=entry, **kw)
    for flags in range(1, 16):                                       # every valid word: only the context is wrong
        rc, msg, untouched = call(flags=flags)
        if flags & 3:
            assert rc == pkg.QMCP_EINVAL and "null context" in msg and untouched, flags
        else:
            assert rc == pkg.QMCP_EINVAL and "neither QMCP_TRACK_IN nor QMCP_TRACK_KEPT" in msg and untouched, flags
    rc, msg, untouched = call(flags=0)
    assert rc == pkg.QMCP_EINVAL and "neither" in msg and untouched
    rc, msg, untouched = call(flags=16 | 1)
    assert rc == pkg.QMCP_EINVAL and "unknown track flags 0x10" in msg and untouched
    rc, msg, untouched = call(columns=False)
    assert rc == pkg.QMCP_EINVAL and "null buffer" in msg and untouched
    for offs in ([1, 1, 2], [0, 2, 1]):
        rc, msg, untouched = call(offs=offs, t0=[1, 2], t1=[3, 4])
        assert rc == pkg.QMCP_EINVAL and "target_offsets" in msg and untouched
    rc, msg, untouched = call(offs=[0, 1, 2], t0=[5, 9], t1=[7, 8])
    assert rc == pkg.QMCP_EINVAL and "start > end" in msg and untouched
    rc, msg, untouched = call(offs=[0, 1, 2])
    assert rc == pkg.QMCP_EINVAL and "null target table" in msg and untouched
    rc, msg, untouched = call(offs=[0, 3, 3], t0=[1, 3, 20], t1=[4, 8, 22])        # a good table: on to the context
    assert "null context" in msg and untouched
    rc, msg, untouched = call(lengths=(50, 0xFFFFFFFF))
    assert rc == pkg.QMCP_ERANGE and "contig 1" in msg and untouched
    rc, msg, untouched = call(flags=0, lengths=(50, 0xFFFFFFFF))                   # the flags are looked at first
    assert rc == pkg.QMCP_EINVAL and "neither" in msg and untouched


def test_without_a_device_a_valid_call_is_enodevice(pkg):
    if pkg.device_count() > 0:
        solver = pkg.Solver(0)
        runs, stats = solver.depth_track([1], [3], [0], [10], 5)
        solver.close()
        assert [tuple(r) for r in runs.tolist()] == [(0, 0, 0, 0, 0, 0), (0, 1, 3, 1, 1, 0), (0, 4, 9, 0, 0, 0)]
        return
    with pytest.raises(pkg.QmcpError) as info:                       # no context without a device, and no CPU fallback
        pkg.Solver(0)
    assert info.value.code == pkg.QMCP_ENODEVICE
    with pytest.raises(ValueError):
        pkg.track_flags(channels=())
    with pytest.raises(ValueError):
        pkg.track_flags(channels=("out",))
    assert pkg.track_flags() == 3 and pkg.track_flags("kept", True, True) == 14 and pkg.track_flags("both") == 3


def _small_call(rng):
    n_contigs = int(rng.integers(1, 5))
    lengths = rng.integers(0, 120, size=n_contigs).astype(np.uint32)
    lengths[rng.random(n_contigs) < 0.2] = rng.choice([0, 1])
    ss, ee, ii = [], [], []
    for c, L in enumerate(lengths.tolist()):
        if L == 0:
            continue
        k = int(rng.integers(0, 40))
        s = rng.integers(0, L, size=k)
        e = np.minimum(s + rng.integers(0, 30, size=k), L - 1)
        if k and rng.random() < 0.5:
            e[0] = L - 1                                             # a read ending on the contig's last position
        ss.append(s); ee.append(e); ii.append(np.full(k, c))
    s = np.concatenate(ss + [np.zeros(2, np.int64)]).astype(np.uint32)
    e = np.concatenate(ee + [np.zeros(2, np.int64)]).astype(np.uint32)
    ids = np.concatenate(ii + [np.full(2, tk.NO_CONTIG)]).astype(np.uint32)
    perm = rng.permutation(s.size)
    return s[perm], e[perm], ids[perm], lengths


def _random_mask(rng, n, p=0.6):
    bits = rng.random(max(n, 1)) < p
    return np.packbits(np.concatenate([bits, np.zeros(-bits.size % 64, bool)]), bitorder="little").view(np.uint64).copy()


def test_the_two_model_forms_agree_and_the_run_bound_holds():
    seen = dict(runs=0, short=0, regions=0, none=0)
    for seed in range(304):
        rng = np.random.default_rng(4000 + seed)
        s, e, ids, lengths = _small_call(rng)
        flags = (1, 2, 3)[seed % 3] | (4 * ((seed // 3) % 4))        # all 12 words with IN or KEPT, ~25 calls each
        mask = None if seed % 5 == 0 else _random_mask(rng, s.size, p=float(rng.choice([0.3, 0.9])))
        kw = dict(keep_mask=mask, flags=flags, depth_cap=int(rng.choice([0, 0, 1, 3])))
        if seed % 2:
            offs, t0, t1 = tm.random_regions(rng, lengths, max_regions=4, max_len=30)
            kw.update(target_offsets=offs, target_starts=t0, target_ends=t1, padding=int(rng.choice([0, 0, 3])))
        M = int(rng.choice([1, 2, 5]))
        want = tk.track_positions(s, e, ids, lengths, M, **kw)
        got = tk.track(s, e, ids, lengths, M, **kw)
        assert got == want, (seed, flags)
        runs, stats = got
        assert stats["n_runs"] == len(runs) <= tk.run_bound(stats, lengths.size), seed
        assert all(a[:2] < b[:2] for a, b in zip(runs, runs[1:])) and all(r[1] <= r[2] for r in runs)
        report = dm.report(s, e, ids, lengths, M, keep_mask=mask,
                           **{k: v for k, v in kw.items() if k.startswith("target") or k == "padding"})
        assert stats["short_positions"] == report["stats"]["deficit_positions"]
        assert stats["scope_positions"] == report["stats"]["scope_positions"]
        seen["runs"] += len(runs)
        seen["short"] += int(stats["short_positions"] > 0)
        seen["regions"] += int(stats["regions_merged"] > 0)
        seen["none"] += int(len(runs) == 0)
    assert seen["runs"] > 3000 and seen["short"] > 100 and seen["regions"] > 100 and seen["none"] > 5, seen


def test_the_event_form_handles_two_huge_contigs_quickly():
    big = 1_200_000_000
    runs, stats = tk.track([5, big - 3, 7], [9, big - 1, 7], [0, 1, 0], [big, big], 1)
    assert runs == [(0, 0, 4, 0, 0, 0), (0, 5, 6, 1, 1, 0), (0, 7, 7, 2, 2, 0), (0, 8, 9, 1, 1, 0), (0, 10, big - 1, 0, 0, 0),
                    (1, 0, big - 4, 0, 0, 0), (1, big - 3, big - 1, 1, 1, 0)]
    assert stats["positions_in_runs"] == stats["scope_positions"] == 2 * big


def _runs_array(pkg, runs):
    return np.array(runs, dtype=pkg.TRACK_RUN_DTYPE) if runs else np.zeros(0, pkg.TRACK_RUN_DTYPE)


def test_write_bedgraph_round_trips_through_profile_from_bedgraph(pkg, tmp_path):
    names = ["chr1", "chrEmpty", "chr2", "chrM"]
    for seed in range(12):
        rng = np.random.default_rng(600 + seed)
        lengths = np.array([int(rng.integers(30, 200)), 0, int(rng.integers(30, 200)), 1], np.uint32)
        n = 60
        ids = rng.choice([0, 2, 3], size=n).astype(np.uint32)
        L = lengths[ids].astype(np.int64)
        s = (rng.random(n) * L).astype(np.int64)
        e = np.minimum(s + rng.integers(0, 40, size=n), L - 1)
        mask = _random_mask(rng, n)
        covs = dm.coverages(s, e, ids, lengths, mask)
        # the same file whatever channels the call compared: runs cut by depth_in are joined again on the kept channel
        texts = []
        for flags in (tk.KEPT, tk.IN | tk.KEPT):
            runs, _ = tk.track(s, e, ids, lengths, 3, keep_mask=mask, flags=flags)
            path = tmp_path / f"kept_{seed}_{flags}.bedgraph"
            lines = pkg.write_bedgraph(path, _runs_array(pkg, runs), names, channel="kept")
            texts.append(path.read_text())
            assert lines == len(texts[-1].split("\n")) - 1
        assert texts[0] == texts[1]
        body = [ln.split("\t") for ln in texts[0].split("\n")[:-1]]
        assert all(len(b) == 4 for b in body) and "chrEmpty" not in {b[0] for b in body}   # zero-length contigs: no line
        for a, b in zip(body, body[1:]):                             # joined: touching neighbours differ in value
            assert not (a[0] == b[0] and a[2] == b[1] and a[3] == b[3])
        offs, r0, r1, caps = pkg.profile_from_bedgraph(tmp_path / f"kept_{seed}_3.bedgraph", names)
        assert offs.tolist()[0] == 0 and offs[2] == offs[1]
        for c in range(4):
            per_position = np.full(int(lengths[c]), -1, np.int64)
            for k in range(int(offs[c]), int(offs[c + 1])):
                per_position[int(r0[k]):int(r1[k]) + 1] = int(caps[k])
            assert np.array_equal(per_position, covs[c][1]), (seed, c)
        # "in" and "both"
        runs, _ = tk.track(s, e, ids, lengths, 3, keep_mask=mask, flags=tk.IN | tk.KEPT)
        pkg.write_bedgraph(tmp_path / "in.bedgraph", _runs_array(pkg, runs), names, channel="in")
        offs, r0, r1, caps = pkg.profile_from_bedgraph(tmp_path / "in.bedgraph", names)
        assert sum(int(caps[k]) * (int(r1[k]) - int(r0[k]) + 1) for k in range(caps.size)) == sum(int(cv[0].sum()) for cv in covs)
        pkg.write_bedgraph(tmp_path / "both.bedgraph", _runs_array(pkg, runs), names, channel="both")
        lines = (tmp_path / "both.bedgraph").read_text().split("\n")
        assert lines[0] == "#chrom\tstart\tend\tdepth_in\tdepth_kept" and lines[-1] == ""
        assert [tuple(ln.split("\t")) for ln in lines[1:-1]] == \
            [(names[r[0]], str(r[1]), str(r[2] + 1), str(r[3]), str(r[4])) for r in _join_both(runs)]
    assert pkg.write_bedgraph(tmp_path / "empty.bedgraph", _runs_array(pkg, []), names) == 0
    assert (tmp_path / "empty.bedgraph").read_text() == ""
    with pytest.raises(ValueError):
        pkg.write_bedgraph(tmp_path / "x.bedgraph", _runs_array(pkg, []), names, channel="short")


def _join_both(runs):
    out = []
    for r in runs:
        if out and out[-1][0] == r[0] and out[-1][2] + 1 == r[1] and out[-1][3:5] == r[3:5]:
            out[-1] = out[-1][:2] + (r[2],) + out[-1][3:]
        else:
            out.append(r)
    return out


def test_a_track_of_the_file_flow_is_refused_where_it_cannot_be_made(pkg, tmp_path):
    import bam_py
    path = tmp_path / "refs.bam"
    bam_py.write_bam(path, [("chr1", 5000), ("chr2", 3000)],
                     [bam_py.pack_record("p0", 0x41, 10, 30, [(50, "M")], 50, ref_id=0),
                      bam_py.pack_record("p0", 0x81, 100, 30, [(50, "M")], 50, ref_id=1)])
    out, track = tmp_path / "out.bam", tmp_path / "depth.bedgraph"
    run = lambda **kw: pkg.downsample_bam("quasi-mcp-hip", path, out, 10, track=track, **kw)
    with pytest.raises(ValueError, match="per_reference"):
        run()
    for kw in (dict(ladder=[5], ladder_out=str(tmp_path / "l{M}.bam")), dict(stratify="strand"), dict(dedup=True),
               dict(profile=tmp_path / "caps.bedgraph")):
        with pytest.raises(ValueError, match="a depth track does not go together with"):
            run(per_reference=True, **kw)
    with pytest.raises(ValueError, match="track_channel"):
        run(per_reference=True, track_channel="short")
    assert not out.exists() and not track.exists()
    # the C++ mirror refuses the same configurations (BamApiConfig::depth_track_filepath)
    err = C.create_string_buffer(1024)
    def entry(per_reference, channel):
        request = pkg._downsample_request(solver_name="quasi-mcp-hip", in_path=path, out_path=tmp_path / "o.bam",
                                          max_coverage=10, amplicon_mode=-1, per_reference=per_reference,
                                          amplicons_by_reference=0, target_padding=0, keep_off_target=0, report_bins=0,
                                          track=track, track_channel=channel, track_cap=0)
        return pkg._host.qmcp_host_downsample_bam(C.byref(request), None, 0, None, None, None, None, None, err, 1024)

    assert entry(0, "kept") == -4 and "per_reference" in err.value.decode()
    assert entry(1, "short") == -4 and "channel" in err.value.decode()
    assert not (tmp_path / "o.bam").exists() and not track.exists()
