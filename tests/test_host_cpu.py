"""CPU-side tests (no GPU): the C ABI library loads and exports every declared symbol, the host-side mirror
(encodings, Scalar) agrees with the golden vectors and the oracle, the product fails loudly without a device,
and the multi-rank sharding/fold plumbing is correct under gloo with world_size 2."""
import json
import os
import re
import subprocess
import sys

import numpy as np
import pytest

from oracle import bls12_381_ref as o

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_abi_exports_every_declared_symbol():
    import bls12_381_amd as b
    from bls12_381_amd import _lib
    hdr = open(os.path.join(ROOT, "include", "bls12_381_hip.h")).read()
    declared = set(re.findall(r"\b(blsgpu_\w+)\s*\(", hdr))
    assert declared, "no declarations parsed"
    assert declared == set(_lib.SIGNATURES), (declared ^ set(_lib.SIGNATURES))
    lib = b.load()                       # binds each symbol; AttributeError if one is missing from the .so
    for name in declared:
        assert hasattr(lib, name), name
    out = subprocess.run(["nm", "-D", "--defined-only", b.LIB_PATH], capture_output=True, text=True).stdout
    exported = set(re.findall(r"\b(blsgpu_\w+)\b", out))
    assert declared <= exported, declared - exported


def test_no_silent_cpu_fallback():
    """Without a HIP device the compute entry points must raise, not fall back to anything."""
    import bls12_381_amd as b
    if b.load().blsgpu_device_count() > 0:
        pytest.skip("a GPU is visible")
    with pytest.raises(b.BlsGpuError):
        b.Context(0)
    src = "".join(open(os.path.join(ROOT, "bls12_381_amd", f)).read() for f in os.listdir(os.path.join(ROOT, "bls12_381_amd")) if f.endswith(".py"))
    assert "import oracle" not in src and "from oracle" not in src, "the product must never import the oracle"


def test_build_inputs_do_not_reach_the_oracle():
    """oracle/ is test infrastructure: neither the run-time package nor anything build() executes may import, hash or read it.
    (1) every generator build() runs (tools/gen_*.py) mentions the oracle only behind its optional --check flag, (2) build()'s own
    source names oracle/ only where it builds the checker (c_oracle.build), (3) the wide-program generator, run in an isolated
    interpreter with the `oracle` package made un-importable, writes a blob byte-identical to the checked run's."""
    tools = os.path.join(ROOT, "tools")
    for f in sorted(os.listdir(tools)):
        if not (f.startswith("gen_") and f.endswith(".py")):
            continue
        lines = open(os.path.join(tools, f)).read().splitlines()
        for i, l in enumerate(lines):
            if re.search(r"^\s*(from|import)\s+oracle\b", l):
                guard = [k for k in range(i - 1, -1, -1) if re.match(r"\s*(if|def|class)\b", lines[k])]
                assert guard and re.match(r"\s*if check\b", lines[guard[0]]), "%s:%d imports the oracle outside `if check:`" % (f, i + 1)
    entry = open(os.path.join(ROOT, "__graft_entry__.py")).read()
    build_src = entry[entry.index("def build("):entry.index("def check_isa(")]
    assert "--check" not in build_src, "build() must not run a generator in its oracle-checking mode"
    mentions = [l for l in build_src.splitlines() if re.search(r"\boracle\b", l) and not l.strip().startswith(("#", '"""'))]
    assert all("c_oracle" in l for l in mentions), mentions          # only `from oracle import c_oracle; c_oracle.build(force)`: building the checker
    os.makedirs(os.path.join(ROOT, "build"), exist_ok=True)
    blocked = os.path.join(ROOT, "build", "no_oracle_site")
    os.makedirs(os.path.join(blocked, "oracle"), exist_ok=True)
    with open(os.path.join(blocked, "oracle", "__init__.py"), "w") as fh:
        fh.write("raise ImportError('the oracle is not a build input')\n")
    gen = os.path.join(tools, "gen_wide_prog.py")
    a, b_ = os.path.join(ROOT, "build", "wide_prog_no_oracle.bin"), os.path.join(ROOT, "build", "wide_prog_checked.bin")
    env = dict(os.environ, PYTHONPATH=blocked)
    subprocess.check_call([sys.executable, gen, "--out", a], env=env, cwd=blocked, stderr=subprocess.DEVNULL)
    subprocess.check_call([sys.executable, gen, "--check", "--out", b_], stderr=subprocess.DEVNULL)
    assert open(a, "rb").read() == open(b_, "rb").read()
    shipped = os.path.join(ROOT, "bls12_381_amd", "wide_prog.bin")
    if os.path.exists(shipped):
        assert open(shipped, "rb").read() == open(a, "rb").read(), "bls12_381_amd/wide_prog.bin is stale: run __graft_entry__.build()"


def test_host_encodings_match_golden(golden_dir):
    """G1Affine / G2Affine (de)serialisation of the host mirror against src/tests/*.dat and the oracle."""
    import bls12_381_amd as b
    for name, cls, usz, dec in (("g1", b.G1Affine, 96, o.g1_from_uncompressed_unchecked), ("g2", b.G2Affine, 192, o.g2_from_uncompressed_unchecked)):
        unc = open(os.path.join(golden_dir, f"{name}_uncompressed_valid_test_vectors.dat"), "rb").read()
        cmp_ = open(os.path.join(golden_dir, f"{name}_compressed_valid_test_vectors.dat"), "rb").read()
        for k in list(range(0, 1000, 37)) + [1, 2, 999]:
            rec = unc[usz * k:usz * (k + 1)]
            pt = cls.from_uncompressed_unchecked(rec)
            assert pt is not None and pt.to_uncompressed() == rec
            assert pt.to_compressed() == cmp_[usz // 2 * k:usz // 2 * (k + 1)]
            assert pt.is_identity() == (k == 0)
            want = dec(rec)
            if name == "g1":
                assert (b.api.limbs_to_fp(pt.xy[:6]), b.api.limbs_to_fp(pt.xy[6:])) == (want[0], want[1]) or k == 0
        assert cls.from_uncompressed_unchecked(b"\xff" * usz) is None              # non-canonical / flags set
        assert cls.generator() == cls.from_uncompressed_unchecked(unc[usz:2 * usz])
        assert (-cls.generator()).to_uncompressed() != cls.generator().to_uncompressed()
        assert cls.identity().to_uncompressed() == unc[:usz]


def test_scalar_mirror():
    import bls12_381_amd as b
    s = b.Scalar(o.R_ORDER + 5)
    assert s.value == 5 and s.to_bytes() == (5).to_bytes(32, "little")
    assert b.Scalar.from_bytes(o.R_ORDER.to_bytes(32, "little")) is None            # not canonical (scalar.rs:256-280)
    assert b.Scalar.from_bytes((o.R_ORDER - 1).to_bytes(32, "little")) == -b.Scalar.one()
    assert b.Scalar.from_bytes_wide(b"\xff" * 64).value == (2 ** 512 - 1) % o.R_ORDER
    assert (s * s.invert()) == b.Scalar.one() and b.Scalar.zero().invert() is None
    assert b.api.scalars_to_bytes([1, b.Scalar(2)]).tolist() == [[1] + [0] * 31, [2] + [0] * 31]


def test_shard_ranges():
    from bls12_381_amd.distributed import shard_range
    for n in (0, 1, 7, 8, 1 << 20, (1 << 24) + 3):
        for w in (1, 2, 3, 8):
            r = [shard_range(n, k, w) for k in range(w)]
            assert r[0][0] == 0 and r[-1][1] == n
            assert all(r[i][1] == r[i + 1][0] for i in range(w - 1))
            assert max(hi - lo for lo, hi in r) - min(hi - lo for lo, hi in r) <= 1


_WORKER = r'''
import os, sys
import numpy as np
sys.path.insert(0, sys.argv[1])
import torch.distributed as dist
from oracle import bls12_381_ref as o
from bls12_381_amd.distributed import sharded_msm, sharded_product
rank, world = int(os.environ["RANK"]), int(os.environ["WORLD_SIZE"])
dist.init_process_group("gloo", rank=rank, world_size=world)
r = o.SplitMix64(5)
n = 11
ks = [r.scalar() for _ in range(n)]; ss = [r.scalar() for _ in range(n)]
pts = [o.g1_to_affine(o.g1_affine_mul(o.G1_GEN, k)) for k in ks]
sb = np.stack([np.frombuffer(s.to_bytes(32, "little"), dtype=np.uint8) for s in ss])
W = lambda x: np.array(o.fp_to_mont_limbs(x), dtype=np.uint64)
def proj_w(p): return np.concatenate([W(p[0]), W(p[1]), W(p[2])])
def w_proj(w): return tuple(o.fp_from_mont_limbs(w[6*i:6*i+6]) for i in range(3))
# the per-rank compute is stood in for by the oracle: this test covers the sharding / all-gather / fold plumbing
def local_msm(lo, hi, s): return proj_w(o.g1_msm(pts[lo:hi], [int.from_bytes(x.tobytes(), "little") for x in s]))
def fold(parts): return proj_w(o.g1_sum([w_proj(p) for p in parts]))
out = sharded_msm(local_msm, fold, sb, world, rank, dist)
want = o.g1_to_affine(o.g1_msm(pts, ss))
assert o.g1_to_affine(w_proj(out)) == want, "sharded MSM differs"
# Fp12 product pattern (multi_miller_loop)
vals = [o.miller_loop(pts[i], o.G2_GEN) for i in range(4)]
F = lambda f: np.concatenate([W(c) for c in o.fp12_flatten(f)])
UF = lambda w: o.fp12_unflatten([o.fp_from_mont_limbs(w[6*i:6*i+6]) for i in range(12)])
import functools
def local_product(lo, hi): return F(functools.reduce(o.fp12_mul, vals[lo:hi], o.FP12_ONE))
def fold12(parts): return F(functools.reduce(o.fp12_mul, [UF(p) for p in parts], o.FP12_ONE))
got = sharded_product(local_product, fold12, 4, world, rank, dist)
assert UF(got) == functools.reduce(o.fp12_mul, vals, o.FP12_ONE)
# independent pairings: index slices, no collective unless the caller asks for the gather (pairings.rs:607-653)
from bls12_381_amd.distributed import sharded_pairings, all_gather_rows
gts = [F(o.final_exponentiation(v)) for v in vals]
def local_pairings(lo, hi): return np.stack(gts[lo:hi]) if hi > lo else np.zeros((0, 72), dtype=np.uint64)
(lo, hi), mine = sharded_pairings(local_pairings, 3, world, rank)
assert mine.shape == (hi - lo, 72) and all(np.array_equal(mine[i], gts[lo + i]) for i in range(hi - lo))
(lo, hi), allv = sharded_pairings(local_pairings, 3, world, rank, gather=True, dist=dist)
assert (lo, hi) == (0, 3) and all(np.array_equal(allv[i], gts[i]) for i in range(3))
# the tensor plumbing of bench.py's RCCL branch, exactly: ONE (world, words) int64 tensor whose unbound rows receive the
# per-rank partials in place, then handed on as one contiguous buffer
import torch
for words in (18, 36, 72):
    gathered = torch.zeros((world, words), dtype=torch.int64)
    row = torch.arange(words, dtype=torch.int64) + 1000 * (rank + 1)
    g = all_gather_rows(gathered, row, dist)
    assert g.data_ptr() == gathered.data_ptr() and g.is_contiguous()
    for rk in range(world):
        assert torch.equal(g[rk], torch.arange(words, dtype=torch.int64) + 1000 * (rk + 1))
# all_gather_partials: a tensor partial stays a tensor on its device (no host round trip), a numpy partial comes back as numpy
from bls12_381_amd.distributed import all_gather_partials
tp = torch.arange(18, dtype=torch.int64) + 7000 * (rank + 1)
gt_ = all_gather_partials(tp, world, dist)
assert isinstance(gt_, torch.Tensor) and gt_.shape == (world, 18) and gt_.device == tp.device and gt_.is_contiguous()
npart = all_gather_partials(tp.numpy().view(np.uint64), world, dist)
assert isinstance(npart, np.ndarray) and npart.dtype == np.uint64
for rk in range(world):
    assert torch.equal(gt_[rk], torch.arange(18, dtype=torch.int64) + 7000 * (rk + 1)) and np.array_equal(npart[rk].view(np.int64), gt_[rk].numpy())
dist.barrier(); dist.destroy_process_group()
print("rank", rank, "ok")
'''


def test_two_rank_gloo_sharding(tmp_path):
    """world_size 2 on CPU (gloo): shard -> per-rank partial -> all-gather -> fold gives the full result on every rank."""
    script = tmp_path / "worker.py"
    script.write_text(_WORKER)
    port = 29500 + os.getpid() % 2000
    procs = []
    for rk in range(2):
        env = dict(os.environ, RANK=str(rk), WORLD_SIZE="2", MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port))
        procs.append(subprocess.Popen([sys.executable, str(script), ROOT], env=env, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True))
    outs = [p.communicate(timeout=240)[0] for p in procs]
    for rk, (p, out) in enumerate(zip(procs, outs)):
        assert p.returncode == 0, out
        assert f"rank {rk} ok" in out


def test_header_is_plain_c():
    """the drop-in boundary must be consumable by a C compiler (cgo / bindgen / ctypes users): C99, no C++, no torch types"""
    import subprocess
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    hdr = os.path.join(root, "include", "bls12_381_hip.h")
    subprocess.check_call(["gcc", "-std=c99", "-Wall", "-Wextra", "-pedantic", "-Werror", "-fsyntax-only", "-x", "c", hdr])
    text = open(hdr).read()
    assert "#include <torch" not in text and "at::" not in text and "std::" not in text


def test_synthetic_scalars_match_the_oracle_stream():
    """the vectorised generator of bench.py / the full-size tests is the SAME SplitMix64 stream as the oracle's scalar-at-a-time
    sampler (32 random bytes, top bit cleared, reject >= r): uniform in [0, r), top bits included"""
    from bls12_381_amd import synthetic as sy
    r = o.SplitMix64(sy.SEED)
    want = [r.scalar() for _ in range(2500)]
    assert sy.to_ints(sy.scalars(2500)) == want
    for n in (0, 1, 2, 1023, 1024, 1025):
        assert sy.to_ints(sy.scalars(n)) == want[:n]
    big = sy.scalars(1 << 16, 7)
    assert all(v < o.R_ORDER for v in sy.to_ints(big[:2000]))
    top = big[:, 31] >> 6                    # bit 254 must occur (r / 2^255 = 0.906: about 45% of the scalars have it set)
    assert 0.40 < float((top == 1).mean()) < 0.50
    a, b = sy.scalars(300, 1), sy.scalars(300, 2)
    assert sy.dot_mod_r(a, b) == sum(x * y for x, y in zip(sy.to_ints(a), sy.to_ints(b))) % o.R_ORDER
    from bls12_381_amd.api import scalars_are_canonical
    assert scalars_are_canonical(big)
    bad = big[:4].copy(); bad[2] = np.frombuffer(o.R_ORDER.to_bytes(32, "little"), dtype=np.uint8)
    assert not scalars_are_canonical(bad)


def test_product_constants_match_reference_literals(kats):
    """bls12_381_amd/csrc/h2c_constants.json (what the library is built from) holds the same numbers as the literals extracted
    from the reference's map_g1.rs / map_g2.rs (tests/golden/ref_kats.json): the product owns its constants, the fixture pins them"""
    import json
    prod = json.load(open(os.path.join(ROOT, "bls12_381_amd", "csrc", "h2c_constants.json")))
    kc = kats["consts"]
    rinv = pow(1 << 384, -1, o.P)
    val = lambda l6: sum(int(v) << (64 * i) for i, v in enumerate(l6)) * rinv % o.P
    for name in ("ISO11_XNUM", "ISO11_XDEN", "ISO11_YNUM", "ISO11_YDEN"):
        assert [int(v, 16) for v in prod["g1"][name]] == [val(v) for v in kc["h2c_g1." + name]], name
    for name in ("SSWU_ELLP_A", "SSWU_ELLP_B", "SSWU_XI", "SQRT_M_XI_CUBED"):
        assert int(prod["g1"][name], 16) == val(kc["h2c_g1." + name][0]), name
    for name in ("ISO3_XNUM", "ISO3_XDEN", "ISO3_YNUM", "ISO3_YDEN", "SSWU_ELLP_A", "SSWU_ELLP_B", "SSWU_XI", "SSWU_RV1", "SSWU_ETAS"):
        flat = [int(c, 16) for v in prod["g2"][name] for c in v]
        assert flat == [val(v) for v in kc["h2c_g2." + name]], name
    gen = open(os.path.join(ROOT, "tools", "gen_consts.py")).read()
    assert "ref_kats" not in gen and "tests\", \"golden" not in gen, "the constants generator must not read anything under tests/"


def test_bench_launch_contract():
    """`python bench.py --gpus N` launched plainly re-executes itself under torch.distributed.run (one rank per GPU) and, for N > 1,
    defaults to ONE 2^24-point MSM sharded N ways (BASELINE configs[3]); checked on the argument logic, no GPU needed"""
    src = open(os.path.join(ROOT, "bench.py")).read()
    assert "torch.distributed.run" in src and "os.execv" in src and '"WORLD_SIZE" not in os.environ' in src
    sys.path.insert(0, ROOT)
    import importlib
    bench = importlib.import_module("bench")
    old = sys.argv
    try:
        sys.argv = ["bench.py", "--gpus", "8"]
        a = bench.parse()
        assert a.log_total == 24 and not a.weak and a.workload == "msm"
        sys.argv = ["bench.py", "--workload", "mixed"]
        assert bench.parse().mixed_log == [22, 22, 18]
    finally:
        sys.argv = old
    from bls12_381_amd.distributed import shard_range
    assert [shard_range(1 << 24, r, 8)[1] - shard_range(1 << 24, r, 8)[0] for r in range(8)] == [1 << 21] * 8


def test_bench_plain_and_full_options_and_output_dumps(kats, tmp_path):
    """a plain `bench.py` run times the steps only (`--full` adds the rest), `--steps` below 1 is refused, and `--dump-outputs` writes
    float64 .npy files whose entries are the bytes of the canonical encodings, exactly"""
    sys.path.insert(0, ROOT)
    import importlib
    bench = importlib.import_module("bench")
    import bls12_381_amd as b
    old = sys.argv
    try:
        sys.argv = ["bench.py", "--gpus", "1", "--steps", "7", "--warmup", "2"]
        a = bench.parse()
        assert a.steps == 7 and a.warmup == 2 and not a.full and a.dump_outputs is None
        sys.argv = ["bench.py", "--full", "--dump-outputs", str(tmp_path)]
        a = bench.parse()
        assert a.full and a.dump_outputs == str(tmp_path)
        for bad in (["--steps", "0"], ["--warmup", "-1"]):
            sys.argv = ["bench.py"] + bad
            with pytest.raises(SystemExit):
                bench.parse()
    finally:
        sys.argv = old
    # Gt = e(G1, G2) from the golden constants: its encoding is the twelve coefficients, 48 big-endian bytes each
    gt = np.array(kats["consts"]["pairings.GT_GENERATOR"], dtype=np.uint64).reshape(72)
    enc = bench.fp12_encoding(b, gt)
    assert enc.dtype == np.uint8 and enc.shape == (576,)
    assert [int.from_bytes(enc[48 * i:48 * i + 48].tobytes(), "big") for i in range(12)] == [o.fp_from_mont_limbs([int(x) for x in gt[6 * i:6 * i + 6]]) for i in range(12)]
    bench.dump_outputs(str(tmp_path / "d"), {"gt": enc})
    back = np.load(str(tmp_path / "d" / "gt.npy"))
    assert back.dtype == np.float64 and np.array_equal(back.astype(np.uint8), enc) and np.array_equal(back, enc.astype(np.float64))


# ---- the Rust side of the boundary (rust/bls12_381-hip): no toolchain here, so it is checked by structure -------------------
_RUST_TYPES = {"c_int": "int", "usize": "size_t", "c_uint": "unsigned", "*mut BlsgpuCtx": "blsgpu_ctx*", "*mut *mut BlsgpuCtx": "blsgpu_ctx**",
               "*mut BlsgpuBases": "blsgpu_bases*", "*const BlsgpuBases": "const blsgpu_bases*", "*mut *mut BlsgpuBases": "blsgpu_bases**",
               "*const u64": "const uint64_t*", "*mut u64": "uint64_t*", "*const u8": "const uint8_t*", "*mut u8": "uint8_t*",
               "*const c_void": "const void*", "*mut c_void": "void*", "*mut f64": "double*", "*mut f32": "float*", "*mut c_uint": "unsigned*",
               "*const c_char": "const char*", "*mut c_char": "char*", "*mut usize": "size_t*", "*const c_int": "const int*",
               "*mut BlsgpuGroup": "blsgpu_group*", "*const BlsgpuGroup": "const blsgpu_group*", "*mut *mut BlsgpuGroup": "blsgpu_group**",
               "*mut BlsgpuG2Prepared": "blsgpu_g2_prepared*", "*const BlsgpuG2Prepared": "const blsgpu_g2_prepared*", "*mut *mut BlsgpuG2Prepared": "blsgpu_g2_prepared**",
               "*const u32": "const uint32_t*", "*mut u32": "uint32_t*", "*const *const c_void": "const void*const*", "*const *mut c_void": "void*const*", "*const usize": "const size_t*",
               "*mut BlsgpuGroupG2Prepared": "blsgpu_group_g2_prepared*", "*const BlsgpuGroupG2Prepared": "const blsgpu_group_g2_prepared*",
               "*mut *mut BlsgpuGroupG2Prepared": "blsgpu_group_g2_prepared**",
               "*mut BlsgpuGroupBases": "blsgpu_group_bases*", "*const BlsgpuGroupBases": "const blsgpu_group_bases*", "*mut *mut BlsgpuGroupBases": "blsgpu_group_bases**"}


def _parse_rust_extern(path):
    src = open(path).read()
    block = re.search(r'extern "C" \{(.*?)\n\}', src, flags=re.S).group(1)
    out = {}
    for m in re.finditer(r"pub fn (\w+)\((.*?)\)(?:\s*->\s*([^;]+))?;", block):
        args = [a.strip() for a in m.group(2).split(",") if a.strip()]
        out[m.group(1)] = ([a.split(":", 1)[1].strip() for a in args], (m.group(3) or "()").strip())
    return out


def test_rust_ffi_matches_header():
    """every `extern "C"` declaration of rust/bls12_381-hip/src/ffi.rs agrees with include/bls12_381_hip.h: same set of symbols,
    same arity, and argument / return types that map onto each other (independent parsers on both sides)"""
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import gen_rust_ffi
    decl = {name: (ret, ps) for name, ret, ps in gen_rust_ffi.parse_header()}
    rust = _parse_rust_extern(os.path.join(ROOT, "rust", "bls12_381-hip", "src", "ffi.rs"))
    from bls12_381_amd import _lib
    assert set(decl) == set(rust) == set(_lib.SIGNATURES), set(decl) ^ set(rust)
    for name, (ret, ps) in decl.items():
        rargs, rret = rust[name]
        assert len(rargs) == len(ps), name
        for (ctype, _), rt in zip(ps, rargs):
            assert _RUST_TYPES[rt] == ctype, (name, ctype, rt)
        assert ("void" if rret == "()" else _RUST_TYPES[rret]) == ret, (name, ret, rret)
        # the ctypes binding has the same arity too
        assert len(_lib.SIGNATURES[name][1]) == len(ps), name
    # the committed file is exactly what the generator produces from the current header
    assert open(os.path.join(ROOT, "rust", "bls12_381-hip", "src", "ffi.rs")).read() == gen_rust_ffi.rust_source()


def test_rust_sources_are_complete():
    """no elided bodies, every ffi:: symbol used is declared, and the trait forwarding of pairings.rs:795-824 is present"""
    base = os.path.join(ROOT, "rust", "bls12_381-hip")
    ffi = _parse_rust_extern(os.path.join(base, "src", "ffi.rs"))
    for rel in ("src/lib.rs", "in-tree/hip.rs"):
        src = open(os.path.join(base, rel)).read()
        assert "/* ..." not in src and "todo!" not in src and "unimplemented!" not in src, rel
        for sym in re.findall(r"ffi::(blsgpu_\w+)", src):
            assert sym in ffi, (rel, sym)
        assert src.count("{") == src.count("}") and src.count("(") == src.count(")"), rel
    lib = open(os.path.join(base, "src", "lib.rs")).read()
    for fn in ("msm_g1", "msm_g2", "mul_batch_g1", "mul_batch_g2", "pairing_batch", "multi_miller_loop", "final_exponentiation", "batch_normalize_g1", "fp12_product", "gt_mul_scalar", "multi_miller_loop_many"):
        assert re.search(r"pub fn %s\b" % fn, lib), fn
    assert "blsgpu_g1_msm_bytes" in lib and "blsgpu_g2_msm_bytes" in lib and "pub struct GpuGroup" in lib and "blsgpu_multi_miller_loop_sharded" in lib
    hip = open(os.path.join(base, "in-tree", "hip.rs")).read()
    for needle in ("impl pairing::Engine for crate::Bls12", "impl pairing::MultiMillerLoop for crate::Bls12", "impl pairing::MillerLoopResult for MillerLoopResult",
                   "pub fn msm_g1", "pub fn msm_g2", "pub fn pairing_batch", "pub fn multi_miller_loop", "pub fn final_exponentiation", "pub fn batch_normalize_g1",
                   "pub fn sum_g1", "pub fn mul_batch_g1", "pub fn mul_batch_g2", "pub const GPU_MIN_PAIRINGS", "impl From<G2Affine> for G2PreparedHip",
                   "pub fn multi_miller_loop_many", "pub struct Group", "impl Drop for Group", "blsgpu_g1_msm_sharded", "blsgpu_multi_miller_loop_sharded", "blsgpu_pairing_batch_sharded"):
        assert needle in hip, needle
    assert os.path.exists(os.path.join(base, "Cargo.toml")) and os.path.exists(os.path.join(base, "build.rs"))


def test_device_code_has_no_folded_subrev_dpp():
    """the shipped library's gfx950 code must not contain `v_subrev_*_dpp` (it miscomputes on this toolchain; see
    pairlane.hip.h::dpp_swap1_sub and __graft_entry__.check_isa)"""
    sys.path.insert(0, ROOT)
    import __graft_entry__ as g
    import bls12_381_amd as b
    g.check_isa(b.LIB_PATH)


def test_scalar_decompositions_against_big_integers():
    """The G1 (GLV) and G2 (psi, base |x|) scalar splits of msm.hip.h, restated branch by branch over Python integers with
    the kernels' own constants (tests/decomp_model.py), reproduce the scalar modulo r and respect the magnitude bounds the
    digit iterators rely on (127-bit halves, 63-bit digits whose top 16-bit window leaves room for the signed-digit carry).
    4*10^5 uniform scalars per group plus every branch boundary; the device kernels are compared with the same candidates in
    tests/test_gpu_parity.py (test_msm_g1_glv_decomposition_boundaries, test_msm_g2_psi_decomposition_boundaries)."""
    from tests import decomp_model as dm
    import random
    rnd = random.Random(0x61C5)
    H = dm.L >> 1
    short = balanced1 = balanced2 = corner = 0
    cands = dm.glv_candidates()
    for i in range(400000 + len(cands)):
        k = cands[i] if i < len(cands) else rnd.randrange(dm.R_ORDER)
        k1, n1, k2, s2, sh = dm.glv_model(k)
        assert dm.glv_value(k1, n1, k2, s2) == k
        assert k1 <= H + 1 and k2 <= H and k1 < (1 << 127) and k2 < (1 << 127)
        assert (k1 >> 112) + 1 <= 1 << 15 and (k2 >> 112) + 1 <= 1 << 15      # top 16-bit window + carry stays a valid signed digit
        short += sh; balanced1 += n1; balanced2 += 1 - s2
        corner += (k1 == 1 and n1 == 1 and s2 == 0)
    assert short and balanced1 and balanced2 and corner                       # every branch of the kernel was exercised
    XH = dm.X_ABS >> 1
    folded = 0
    cands = dm.gls_candidates()
    for i in range(200000 + len(cands)):
        k = cands[i] if i < len(cands) else rnd.randrange(dm.R_ORDER)
        t = dm.gls_model(k)
        assert dm.gls_value(t) == k
        assert all(m <= XH + 1 and m < (1 << 63) for m, _ in t)
        assert all((m >> 48) + 1 <= 1 << 15 for m, _ in t)
        folded += t[2][0] > XH
    assert folded >= 0


def test_bench_line_is_compact_and_ends_with_the_pairing_half_of_the_metric():
    """the driver keeps the last ~8 000 characters of stdout: the compact line built from a FULL record (round 4's, with every note and
    table in it) stays under 6 000 characters, is valid JSON with the contract's keys, and its last 2 000 characters carry the
    2^16-pairing figure, its roofline fraction and its CPU baseline (round-4 review: they had been pushed out of the record)"""
    sys.path.insert(0, ROOT)
    import bench
    full = json.load(open(os.path.join(ROOT, "profiles", "r04_bench_default_n1.json")))
    # the round-5 additions, with long notes, as bench.py now produces them
    full["extras"]["verification_equations"]["prepared"] = {"n": 16384, "ms": 7.5, "equations_per_s": 2.2e6, "speedup_over_unprepared": 1.4, "unprepared_same_equations_ms": 10.5,
                                                            "paths_agree": True, "gpu_result_matches": True, "note": "x" * 900,
                                                            "roofline": {"bound": "int-valu", "kernel": "k", "achieved": 14.2, "peak": 37.0, "unit": "TMAC32/s", "frac": 0.38, "traffic": None},
                                                            "cpu_baseline": {"value": 9000.0, "unit": "equations/s", "cores": 16, "kind": "port", "sample": "y" * 400},
                                                            "n65536": {"ms": 27.0, "equations_per_s": 2.4e6, "speedup_over_unprepared": 1.37, "roofline": {"frac": 0.42}}}
    full["group_path"] = {"members": 8, "ms_per_step": 6.0, "value": 2.8e9, "note": "z" * 500}
    s = json.dumps(bench.slim_line(full))
    assert len(s) < 6000, len(s)
    back = json.loads(s)
    for k in ("metric", "value", "unit", "n_gpus", "steps", "warmup", "ms_per_step", "higher_is_better", "scaling", "vs_baseline", "dtype", "data", "config", "roofline", "cpu_baseline"):
        assert k in back, k
    assert set(("bound", "achieved", "peak", "unit", "frac", "traffic")) <= set(back["roofline"]) and back["roofline"]["frac"] == pytest.approx(full["roofline"]["frac"], rel=1e-4)
    assert set(("value", "unit", "cores", "kind", "sample")) <= set(back["cpu_baseline"])
    tail = s[-2000:]
    for needle in ('"pairing_frac"', '"pairing_ms"', '"pairings_per_s"', '"cpu_baseline_pairing"', '"mml_frac"', '"equations_frac"', '"prepared_equations_speedup"'):
        assert needle in tail, needle
    assert back["pairing_ms"] == pytest.approx(full["extras"]["pairing_batch"]["ms"], rel=1e-4)
    assert back["pairing_batch"]["roofline"]["frac"] == pytest.approx(full["extras"]["pairing_batch"]["roofline"]["frac"], rel=1e-4)
    # round 6: the record as bench.py now writes it (per-leg timing blocks with kernel_ms, clocks, counter traffic and VALU issue fractions on every leg)
    full6 = json.load(open(os.path.join(ROOT, "profiles", "r06_bench_default_n1_detail.json")))
    s6 = json.dumps(bench.slim_line(full6))
    assert len(s6) < 7700, len(s6)
    back6 = json.loads(s6)
    tail6 = s6[-2000:]
    for needle in ('"pairing_frac"', '"pairing_ms"', '"pairings_per_s"', '"cpu_baseline_pairing"', '"mml_frac"', '"prepared_equations_speedup"', '"kernel_ms"'):
        assert needle in tail6, needle
    assert "timing" in back6["pairing_batch"] and set(("min", "med", "max", "kernel_ms")) <= set(back6["pairing_batch"]["timing"])
    assert back6["roofline"]["traffic"] and all("roofline" not in v or v["roofline"].get("traffic") for v in back6["extras"].values() if isinstance(v, dict) and "roofline" in v)
    assert list(back)[-1] in ("prepared_equations_speedup", "equations_frac")


def test_profile_digests_are_stamped_only_on_the_files_a_tool_wrote(tmp_path, monkeypatch):
    """bench.py marks a leg's committed counter traffic STALE when the kernel sources changed since collection (tools/srcdigest.py).  A summarising
    tool must therefore stamp only the files whose counters it has just taken from a run of this checkout: stamping every file of the round would
    vouch for counters that were not re-collected (round 6: it did)."""
    import importlib, json, sys
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    sd = importlib.import_module("srcdigest")
    prof = tmp_path / "profiles"; prof.mkdir()
    for tag in ("msm", "pairing", "hash_to_g2"):
        (prof / ("r99_%s_pmc.json" % tag)).write_text(json.dumps({"source_digest": "old", "counters": {}}))
    monkeypatch.setattr(sd, "ROOT", str(tmp_path))
    sd.stamp("r99", ["msm"])
    got = {tag: json.loads((prof / ("r99_%s_pmc.json" % tag)).read_text())["source_digest"] for tag in ("msm", "pairing", "hash_to_g2")}
    assert got["msm"] == sd.source_digest("msm") != "old" and got["pairing"] == "old" and got["hash_to_g2"] == "old"
    # the digest covers the field arithmetic every kernel shares and the family's own sources
    assert sd.source_digest("msm") != sd.source_digest("pairing")
