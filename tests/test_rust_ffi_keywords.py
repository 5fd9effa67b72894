"""No parameter of the generated Rust declarations (rust/bls12_381-hip/src/ffi.rs) may be a bare Rust keyword: `in: *const u64` is a parse
error that stops the whole `extern "C"` block from compiling, and there is no Rust toolchain here to say so.  The generator writes such a
name as a raw identifier (`r#type`); this checks the committed file and the generator's own output for every C parameter name."""
import os
import re
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))

# https://doc.rust-lang.org/reference/keywords.html: strict, reserved (2018+) -- stated here independently of the generator's own list
KEYWORDS = set("""as break const continue crate else enum extern false fn for if impl in let loop match mod move mut pub ref return self Self
static struct super trait true type unsafe use where while async await dyn abstract become box do final macro override priv typeof unsized
virtual yield try""".split())


def _param_names(src):
    block = re.search(r'extern "C" \{(.*?)\n\}', src, flags=re.S).group(1)
    for m in re.finditer(r"pub fn (\w+)\((.*?)\)", block):
        for arg in m.group(2).split(","):
            if arg.strip():
                yield m.group(1), arg.split(":", 1)[0].strip()


def test_no_parameter_is_a_bare_rust_keyword():
    import gen_rust_ffi
    committed = open(os.path.join(ROOT, "rust", "bls12_381-hip", "src", "ffi.rs")).read()
    for src in (committed, gen_rust_ffi.rust_source()):
        names = list(_param_names(src))
        assert len(names) > 500
        bad = [(fn, n) for fn, n in names if n in KEYWORDS]
        assert not bad, bad
        assert all(re.fullmatch(r"(r#)?[A-Za-z_]\w*", n) for _, n in names)


def test_the_generator_escapes_a_keyword_parameter():
    """a header parameter named like a keyword comes out as a raw identifier"""
    import gen_rust_ffi
    assert KEYWORDS <= set(gen_rust_ffi.RUST_KEYWORDS)
    src = gen_rust_ffi.rust_source([("blsgpu_probe", "int", [("const uint64_t*", "in"), ("int", "type"), ("size_t", "n")])])
    assert [n for _, n in _param_names(src)] == ["r#in", "r#type", "n"]
