//! MI355X back end for the hot path of `bls12_381` through the C ABI of `libblsgpu.so` (include/bls12_381_hip.h).
//!
//! This crate is the OUT-OF-TREE binding: it can only see what `bls12_381` 0.8 exports, so group elements cross the
//! boundary in the crate's public encodings (`to_uncompressed` / `from_uncompressed_unchecked`, `Scalar::to_bytes`) and
//! target-group values -- `Gt` has no public constructor or encoding -- stay as the 72 canonical Montgomery limbs the
//! reference keeps inside `Gt(Fp12)` (`GtLimbs`; equality of limbs is equality of group elements because `Fp` is always
//! fully reduced, src/fp.rs:361-379).  The limb-level module that returns the crate's own `Gt` / `MillerLoopResult` and
//! forwards `pairing::Engine` / `MultiMillerLoop` for `Bls12` lives in `in-tree/hip.rs` (it needs `pub(crate)` fields).
//!
//! Reference semantics, by entry point:
//!   msm_g1 / msm_g2           bases.iter().zip(scalars).map(|(p, s)| p * s).sum()      src/g1.rs:573-579,754-774,161-171
//!   pairing_batch             pairing(p_i, q_i) for every i                             src/pairings.rs:607-653
//!   multi_miller_loop         multi_miller_loop(&[(p_i, prepared q_i)])                 src/pairings.rs:554-603
//!   final_exponentiation      MillerLoopResult::final_exponentiation                    src/pairings.rs:48-176
//!   batch_normalize_g1        G1Projective::batch_normalize                             src/g1.rs:806-839
//!   ntt_g1 / ntt_g2           the radix-2 group FFT a caller writes over `ROOT_OF_UNITY`                src/scalar.rs:193-205
//!   multi_miller_loop_many    multi_miller_loop(terms_s).final_exponentiation() for every equation s    src/pairings.rs:554-603, 48-176
//!   GpuGroup::*               the same operations sharded over the GPUs of the node (folds: `Sum`, `MillerLoopResult +`)
//! Hot-path functions of the reference are infallible; here a HIP failure or a bad argument is an `Err(Error)` and the
//! caller decides (fall back to the CPU expression above, or propagate).  The library itself never computes on the CPU.
#![allow(clippy::missing_safety_doc)]

pub mod ffi;

use bls12_381::{G1Affine, G1Projective, G2Affine, G2Projective, Scalar};
use core::ffi::{c_int, c_void, CStr};
use group::Curve;

/// Error of a library call: the status code and `blsgpu_last_error()`.
#[derive(Debug, Clone)]
pub struct Error { pub code: i32, pub message: String }

fn check(rc: c_int) -> Result<(), Error> {
    if rc == ffi::BLSGPU_OK { return Ok(()); }
    let message = unsafe {
        let p = ffi::blsgpu_last_error();
        if p.is_null() { String::new() } else { CStr::from_ptr(p).to_string_lossy().into_owned() }
    };
    Err(Error { code: rc, message })
}

/// One context = one device with its streams and scratch memory.  Not `Sync`: use one per host thread.
pub struct Gpu { ctx: *mut ffi::BlsgpuCtx }
unsafe impl Send for Gpu {}

impl Gpu {
    pub fn new(device: i32) -> Result<Gpu, Error> {
        let mut ctx = core::ptr::null_mut();
        check(unsafe { ffi::blsgpu_create(device, &mut ctx) })?;
        Ok(Gpu { ctx })
    }
    pub fn device_count() -> i32 { unsafe { ffi::blsgpu_device_count() } }
    pub fn raw(&self) -> *mut ffi::BlsgpuCtx { self.ctx }
    /// waits for everything queued on this context; also reports a non-canonical scalar seen by an asynchronous MSM
    pub fn synchronize(&self) -> Result<(), Error> { check(unsafe { ffi::blsgpu_synchronize(self.ctx) }) }
}
impl Drop for Gpu { fn drop(&mut self) { unsafe { ffi::blsgpu_destroy(self.ctx) } } }

/// The 72 canonical Montgomery limbs of a `Gt` / `MillerLoopResult` in struct order c0.c0.c0 .. c1.c2.c1 (src/fp12.rs:13-16).
#[derive(Clone, Copy, PartialEq, Eq, Debug)]
pub struct GtLimbs(pub [u64; 72]);

fn scalar_bytes(scalars: &[Scalar]) -> Vec<u8> {
    let mut s = Vec::with_capacity(scalars.len() * 32);
    for k in scalars { s.extend_from_slice(&k.to_bytes()); }          // src/scalar.rs:284-296: canonical, little endian
    s
}
fn g1_bytes(points: &[G1Affine]) -> Vec<u8> {
    let mut b = Vec::with_capacity(points.len() * 96);
    for p in points { b.extend_from_slice(&p.to_uncompressed()); }    // src/g1.rs:246-260
    b
}
fn g2_bytes(points: &[G2Affine]) -> Vec<u8> {
    let mut b = Vec::with_capacity(points.len() * 192);
    for p in points { b.extend_from_slice(&p.to_uncompressed()); }    // src/g2.rs:284-299
    b
}

/// Drop-in for `bases.iter().zip(scalars).map(|(p, s)| p * s).sum::<G1Projective>()`.
pub fn msm_g1(gpu: &Gpu, bases: &[G1Affine], scalars: &[Scalar]) -> Result<G1Projective, Error> {
    assert_eq!(bases.len(), scalars.len());
    let (b, s) = (g1_bytes(bases), scalar_bytes(scalars));
    let mut out = [0u8; 96];
    check(unsafe { ffi::blsgpu_g1_msm_bytes(gpu.ctx, b.as_ptr(), s.as_ptr(), bases.len(), out.as_mut_ptr()) })?;
    // the library returns a valid encoding of a subgroup point; `unchecked` skips a second subgroup check
    let aff = Option::<G1Affine>::from(G1Affine::from_uncompressed_unchecked(&out)).expect("libblsgpu returned an invalid G1 encoding");
    Ok(G1Projective::from(aff))
}

/// Drop-in for the same expression over G2 (src/g2.rs:626-632,825-845,162-172).
pub fn msm_g2(gpu: &Gpu, bases: &[G2Affine], scalars: &[Scalar]) -> Result<G2Projective, Error> {
    assert_eq!(bases.len(), scalars.len());
    let (b, s) = (g2_bytes(bases), scalar_bytes(scalars));
    let mut out = [0u8; 192];
    check(unsafe { ffi::blsgpu_g2_msm_bytes(gpu.ctx, b.as_ptr(), s.as_ptr(), bases.len(), out.as_mut_ptr()) })?;
    let aff = Option::<G2Affine>::from(G2Affine::from_uncompressed_unchecked(&out)).expect("libblsgpu returned an invalid G2 encoding");
    Ok(G2Projective::from(aff))
}

/// Decode uncompressed encodings into the wire limbs of the ABI (x | y Montgomery limbs + infinity bytes) on the GPU.
fn g1_wire(gpu: &Gpu, points: &[G1Affine]) -> Result<(Vec<u64>, Vec<u8>), Error> {
    let n = points.len();
    let bytes = g1_bytes(points);
    let (mut xy, mut inf, mut ok) = (vec![0u64; n * 12], vec![0u8; n], vec![0u8; n]);
    check(unsafe { ffi::blsgpu_g1_from_bytes_batch(gpu.ctx, bytes.as_ptr(), n, 0, 0, xy.as_mut_ptr(), inf.as_mut_ptr(), ok.as_mut_ptr()) })?;
    debug_assert!(ok.iter().all(|&o| o == 1));
    Ok((xy, inf))
}
fn g2_wire(gpu: &Gpu, points: &[G2Affine]) -> Result<(Vec<u64>, Vec<u8>), Error> {
    let n = points.len();
    let bytes = g2_bytes(points);
    let (mut xy, mut inf, mut ok) = (vec![0u64; n * 24], vec![0u8; n], vec![0u8; n]);
    check(unsafe { ffi::blsgpu_g2_from_bytes_batch(gpu.ctx, bytes.as_ptr(), n, 0, 0, xy.as_mut_ptr(), inf.as_mut_ptr(), ok.as_mut_ptr()) })?;
    debug_assert!(ok.iter().all(|&o| o == 1));
    Ok((xy, inf))
}
/// Drop-in for `points.iter().zip(scalars).map(|(p, s)| p * s).collect::<Vec<G1Projective>>()` -- `Mul<&Scalar>` over
/// slices (src/g1.rs:573-579, 754-774): decode on the device, N variable-base multiplications in one launch, one batched
/// affine conversion, encode; exact for every curve point (no subgroup precondition).
pub fn mul_batch_g1(gpu: &Gpu, points: &[G1Affine], scalars: &[Scalar]) -> Result<Vec<G1Projective>, Error> {
    assert_eq!(points.len(), scalars.len());
    let n = points.len();
    let ((xy, inf), s) = (g1_wire(gpu, points)?, scalar_bytes(scalars));
    let (mut xyz, mut axy, mut ainf, mut enc) = (vec![0u64; n * 18], vec![0u64; n * 12], vec![0u8; n], vec![0u8; n * 96]);
    check(unsafe { ffi::blsgpu_g1_mul_batch(gpu.ctx, xy.as_ptr(), inf.as_ptr(), s.as_ptr(), n, xyz.as_mut_ptr()) })?;
    check(unsafe { ffi::blsgpu_g1_batch_normalize(gpu.ctx, xyz.as_ptr(), n, axy.as_mut_ptr(), ainf.as_mut_ptr()) })?;
    check(unsafe { ffi::blsgpu_g1_to_bytes_batch(gpu.ctx, axy.as_ptr(), ainf.as_ptr(), n, 0, enc.as_mut_ptr()) })?;
    Ok(enc.chunks_exact(96).map(|c| {
        let mut b = [0u8; 96]; b.copy_from_slice(c);
        G1Projective::from(Option::<G1Affine>::from(G1Affine::from_uncompressed_unchecked(&b)).expect("libblsgpu returned an invalid G1 encoding"))
    }).collect())
}
/// the same over G2 (src/g2.rs:626-632, 825-845)
pub fn mul_batch_g2(gpu: &Gpu, points: &[G2Affine], scalars: &[Scalar]) -> Result<Vec<G2Projective>, Error> {
    assert_eq!(points.len(), scalars.len());
    let n = points.len();
    let ((xy, inf), s) = (g2_wire(gpu, points)?, scalar_bytes(scalars));
    let (mut xyz, mut axy, mut ainf, mut enc) = (vec![0u64; n * 36], vec![0u64; n * 24], vec![0u8; n], vec![0u8; n * 192]);
    check(unsafe { ffi::blsgpu_g2_mul_batch(gpu.ctx, xy.as_ptr(), inf.as_ptr(), s.as_ptr(), n, xyz.as_mut_ptr()) })?;
    check(unsafe { ffi::blsgpu_g2_batch_normalize(gpu.ctx, xyz.as_ptr(), n, axy.as_mut_ptr(), ainf.as_mut_ptr()) })?;
    check(unsafe { ffi::blsgpu_g2_to_bytes_batch(gpu.ctx, axy.as_ptr(), ainf.as_ptr(), n, 0, enc.as_mut_ptr()) })?;
    Ok(enc.chunks_exact(192).map(|c| {
        let mut b = [0u8; 192]; b.copy_from_slice(c);
        G2Projective::from(Option::<G2Affine>::from(G2Affine::from_uncompressed_unchecked(&b)).expect("libblsgpu returned an invalid G2 encoding"))
    }).collect())
}
/// `Fp::one()` in Montgomery limbs (R mod p, src/fp.rs:83-90): the Z of an affine point lifted to a projective wire point
const FP_ONE: [u64; 6] = [0x760900000002fffd, 0xebf4000bc40c0002, 0x5f48985753c758ba, 0x77ce585370525745, 0x5c071a97a256ec6d, 0x15f65ec3fa80e493];
/// affine wire limbs + infinity bytes -> projective wire points X | Y | Z (Z = 1; the identity is (0 : 1 : 0)); w = limbs per coordinate
fn lift_wire(xy: &[u64], inf: &[u8], w: usize) -> Vec<u64> {
    let mut xyz = vec![0u64; inf.len() * 3 * w];
    for (i, &f) in inf.iter().enumerate() {
        let p = &mut xyz[i * 3 * w..(i + 1) * 3 * w];
        if f != 0 { p[w..w + 6].copy_from_slice(&FP_ONE); continue; }
        p[..2 * w].copy_from_slice(&xy[i * 2 * w..(i + 1) * 2 * w]);
        p[2 * w..2 * w + 6].copy_from_slice(&FP_ONE);
    }
    xyz
}
/// Radix-2 transform over G1 elements, `k` vectors of `points.len() / k` points each (a power of two) in one call:
/// `Y[m] = sum_j P[j] * w^(jm)` with `w = Scalar::ROOT_OF_UNITY^(2^(32 - log_n))` (src/scalar.rs:193-205), the inverse scaled by `n^-1` --
/// what a caller writes as a group FFT over `G1Projective`, e.g. a monomial SRS into its Lagrange form.  Every point must lie in the
/// prime-order subgroup, which every `G1Affine` the crate's checked constructors hand out does.
pub fn ntt_g1(gpu: &Gpu, points: &[G1Affine], k: usize, inverse: bool) -> Result<Vec<G1Projective>, Error> {
    let n = points.len();
    assert!(k > 0 && n % k == 0 && (n / k).is_power_of_two());
    let (xy, inf) = g1_wire(gpu, points)?;
    let mut xyz = lift_wire(&xy, &inf, 6);
    let (mut axy, mut ainf, mut enc) = (vec![0u64; n * 12], vec![0u8; n], vec![0u8; n * 96]);
    check(unsafe { ffi::blsgpu_g1_ntt_many(gpu.ctx, xyz.as_mut_ptr(), (n / k).trailing_zeros() as c_int, k, inverse as c_int) })?;
    check(unsafe { ffi::blsgpu_g1_batch_normalize(gpu.ctx, xyz.as_ptr(), n, axy.as_mut_ptr(), ainf.as_mut_ptr()) })?;
    check(unsafe { ffi::blsgpu_g1_to_bytes_batch(gpu.ctx, axy.as_ptr(), ainf.as_ptr(), n, 0, enc.as_mut_ptr()) })?;
    Ok(enc.chunks_exact(96).map(|c| {
        let mut b = [0u8; 96]; b.copy_from_slice(c);
        G1Projective::from(Option::<G1Affine>::from(G1Affine::from_uncompressed_unchecked(&b)).expect("libblsgpu returned an invalid G1 encoding"))
    }).collect())
}
/// the same over G2
pub fn ntt_g2(gpu: &Gpu, points: &[G2Affine], k: usize, inverse: bool) -> Result<Vec<G2Projective>, Error> {
    let n = points.len();
    assert!(k > 0 && n % k == 0 && (n / k).is_power_of_two());
    let (xy, inf) = g2_wire(gpu, points)?;
    let mut xyz = lift_wire(&xy, &inf, 12);
    let (mut axy, mut ainf, mut enc) = (vec![0u64; n * 24], vec![0u8; n], vec![0u8; n * 192]);
    check(unsafe { ffi::blsgpu_g2_ntt_many(gpu.ctx, xyz.as_mut_ptr(), (n / k).trailing_zeros() as c_int, k, inverse as c_int) })?;
    check(unsafe { ffi::blsgpu_g2_batch_normalize(gpu.ctx, xyz.as_ptr(), n, axy.as_mut_ptr(), ainf.as_mut_ptr()) })?;
    check(unsafe { ffi::blsgpu_g2_to_bytes_batch(gpu.ctx, axy.as_ptr(), ainf.as_ptr(), n, 0, enc.as_mut_ptr()) })?;
    Ok(enc.chunks_exact(192).map(|c| {
        let mut b = [0u8; 192]; b.copy_from_slice(c);
        G2Projective::from(Option::<G2Affine>::from(G2Affine::from_uncompressed_unchecked(&b)).expect("libblsgpu returned an invalid G2 encoding"))
    }).collect())
}
/// `Scalar`s -> the four Montgomery limbs each that the Fr entry points take (`Scalar::to_bytes`, src/scalar.rs:284-296, converted on the GPU)
fn scalar_limbs(gpu: &Gpu, scalars: &[Scalar]) -> Result<Vec<u64>, Error> {
    let (bytes, mut limbs) = (scalar_bytes(scalars), vec![0u64; scalars.len() * 4]);
    check(unsafe { ffi::blsgpu_fr_from_bytes(gpu.ctx, bytes.as_ptr(), scalars.len(), limbs.as_mut_ptr(), std::ptr::null_mut()) })?;
    Ok(limbs)
}
fn limbs_scalars(gpu: &Gpu, limbs: &[u64]) -> Result<Vec<Scalar>, Error> {
    let n = limbs.len() / 4;
    let mut bytes = vec![0u8; n * 32];
    check(unsafe { ffi::blsgpu_fr_to_bytes(gpu.ctx, limbs.as_ptr(), n, bytes.as_mut_ptr(), std::ptr::null_mut()) })?;
    Ok(bytes.chunks_exact(32).map(|c| {
        let mut b = [0u8; 32]; b.copy_from_slice(c);
        Option::<Scalar>::from(Scalar::from_bytes(&b)).expect("libblsgpu returned a non-canonical Scalar")
    }).collect())
}
/// The recurrences of `blsgpu_fr_scan_many` over `k` rows of `values.len() / k` scalars each, in one call.
#[derive(Clone, Copy, PartialEq, Eq, Debug)]
pub enum FrScan { Sum = 0, Product = 1, Horner = 2 }
/// `Sum` / `Product`: running sums / products along each row (`exclusive`: of the elements before each position, starting from 0 / 1).
/// `Horner`: row v holds the coefficients of p_v (index i = X^i), `points[v]` = z; the result row is p_v(z) followed by the coefficients of
/// the quotient (p_v(X) - p_v(z)) / (X - z) -- what a caller writes as a loop `h = c[i] + z * h` from the top coefficient down.
pub fn fr_scan(gpu: &Gpu, op: FrScan, values: &[Scalar], k: usize, points: &[Scalar], exclusive: bool) -> Result<Vec<Scalar>, Error> {
    if values.is_empty() { return Ok(Vec::new()); }
    assert!(k > 0 && values.len() % k == 0);
    assert!(op != FrScan::Horner || (points.len() == k && !exclusive));
    let input = scalar_limbs(gpu, values)?;
    let pts = if op == FrScan::Horner { scalar_limbs(gpu, points)? } else { Vec::new() };
    let mut out = vec![0u64; input.len()];
    check(unsafe {
        ffi::blsgpu_fr_scan_many(gpu.ctx, op as c_int, exclusive as c_int, input.as_ptr(), values.len() / k, k,
                                 if pts.is_empty() { std::ptr::null() } else { pts.as_ptr() }, out.as_mut_ptr())
    })?;
    limbs_scalars(gpu, &out)
}
/// Drop-in for `values.iter().map(|v| v.invert())` (src/scalar.rs:573-628) by Montgomery's trick: `None` where the input is zero.
pub fn fr_batch_invert(gpu: &Gpu, values: &[Scalar]) -> Result<Vec<Option<Scalar>>, Error> {
    if values.is_empty() { return Ok(Vec::new()); }
    let input = scalar_limbs(gpu, values)?;
    let (mut out, mut flags) = (vec![0u64; input.len()], vec![0u8; values.len()]);
    check(unsafe { ffi::blsgpu_fr_batch_invert(gpu.ctx, input.as_ptr(), values.len(), out.as_mut_ptr(), flags.as_mut_ptr()) })?;
    Ok(limbs_scalars(gpu, &out)?.into_iter().zip(flags).map(|(s, f)| if f != 0 { Some(s) } else { None }).collect())
}
/// The accumulator column of a permutation argument (`blsgpu_fr_grand_product`): column sets of `c` tables of `k` rows, packed
/// (`num_a.len() = c * k * len`); an empty `num_b` / `den_b` drops that side's beta term.  With n_j = num_a_j + beta num_b_j + gamma and
/// d_j = den_a_j + beta den_b_j + gamma: f[i] = prod_j n_j[i] * (prod_j d_j[i])^-1 (0 where a d_j[i] is zero), and the result is the
/// running product of f along each row (`exclusive`: starting from 1).  The flags are `false` where a denominator factor was zero.
///
/// # Panics
/// If `c` or `k` is zero, a set's length is not a multiple of `c * k`, or the sets differ in length (the C++ mirror throws and the C ABI
/// cannot see slice lengths at all: the sizes are checked here, before the call).  What the library itself refuses comes back as `Err`.
pub fn fr_grand_product(gpu: &Gpu, c: usize, k: usize, num_a: &[Scalar], num_b: &[Scalar], den_a: &[Scalar], den_b: &[Scalar], beta: &Scalar, gamma: &Scalar,
                        exclusive: bool) -> Result<(Vec<Scalar>, Vec<bool>), Error> {
    assert!(c > 0 && k > 0 && num_a.len() % (c * k) == 0 && den_a.len() == num_a.len());
    assert!((num_b.is_empty() || num_b.len() == num_a.len()) && (den_b.is_empty() || den_b.len() == num_a.len()));
    let total = num_a.len() / c;
    if total == 0 { return Ok((Vec::new(), Vec::new())); }
    let lim = |v: &[Scalar]| if v.is_empty() { Ok(Vec::new()) } else { scalar_limbs(gpu, v) };
    let (na, nb, da, db) = (lim(num_a)?, lim(num_b)?, lim(den_a)?, lim(den_b)?);
    let chal = scalar_limbs(gpu, &[*beta, *gamma])?;
    let opt = |v: &Vec<u64>| if v.is_empty() { std::ptr::null() } else { v.as_ptr() };
    let (mut out, mut flags) = (vec![0u64; total * 4], vec![0u8; total]);
    check(unsafe {
        ffi::blsgpu_fr_grand_product(gpu.ctx, exclusive as c_int, c as c_int, na.as_ptr(), opt(&nb), da.as_ptr(), opt(&db), chal.as_ptr(), total / k, k, out.as_mut_ptr(),
                                     flags.as_mut_ptr())
    })?;
    Ok((limbs_scalars(gpu, &out)?, flags.into_iter().map(|f| f != 0).collect()))
}
/// The accumulator column of a log-derivative lookup argument (`blsgpu_fr_frac_sum`): f[i] = sum_j mult_j[i] / (gamma + den_a_j[i] +
/// beta den_b_j[i]) with a zero denominator's term dropped, and the running sum of f along each row.  An empty `mult` means every
/// multiplicity is 1 (signs belong in `mult`), an empty `den_b` drops the beta term.  Sets and flags as for `fr_grand_product`.
///
/// # Panics
/// As `fr_grand_product`: on mismatched set sizes, before the call.
pub fn fr_frac_sum(gpu: &Gpu, c: usize, k: usize, mult: &[Scalar], den_a: &[Scalar], den_b: &[Scalar], beta: &Scalar, gamma: &Scalar, exclusive: bool)
                   -> Result<(Vec<Scalar>, Vec<bool>), Error> {
    assert!(c > 0 && k > 0 && den_a.len() % (c * k) == 0);
    assert!((mult.is_empty() || mult.len() == den_a.len()) && (den_b.is_empty() || den_b.len() == den_a.len()));
    let total = den_a.len() / c;
    if total == 0 { return Ok((Vec::new(), Vec::new())); }
    let lim = |v: &[Scalar]| if v.is_empty() { Ok(Vec::new()) } else { scalar_limbs(gpu, v) };
    let (m, da, db) = (lim(mult)?, lim(den_a)?, lim(den_b)?);
    let chal = scalar_limbs(gpu, &[*beta, *gamma])?;
    let opt = |v: &Vec<u64>| if v.is_empty() { std::ptr::null() } else { v.as_ptr() };
    let (mut out, mut flags) = (vec![0u64; total * 4], vec![0u8; total]);
    check(unsafe {
        ffi::blsgpu_fr_frac_sum(gpu.ctx, exclusive as c_int, c as c_int, opt(&m), da.as_ptr(), opt(&db), chal.as_ptr(), total / k, k, out.as_mut_ptr(), flags.as_mut_ptr())
    })?;
    Ok((limbs_scalars(gpu, &out)?, flags.into_iter().map(|f| f != 0).collect()))
}
/// How a row of evaluations is ordered: `D[i] = w^i`, or `D[i] = w^bitrev(i)` (how blob formats store their rows).
#[derive(Clone, Copy, PartialEq, Eq, Debug)]
pub enum FrOrder { Natural = 0, BitReversed = 1 }
fn fr_bary_log_n(len: usize, k: usize, points: usize) -> c_int {
    assert!(k > 0 && len > 0 && len % k == 0 && points == k);
    let n = len / k;
    assert!(n.is_power_of_two());
    n.trailing_zeros() as c_int
}
/// `k` polynomials in evaluation form, row v = p_v on the `evals.len() / k` = 2^log_n roots of unity in the given order: returns
/// `p_v(points[v])` (`blsgpu_fr_bary_eval_many`).  A point inside the domain is handled exactly.
pub fn fr_bary_eval(gpu: &Gpu, evals: &[Scalar], k: usize, points: &[Scalar], order: FrOrder) -> Result<Vec<Scalar>, Error> {
    if evals.is_empty() && k == 0 { return Ok(Vec::new()); }
    let log_n = fr_bary_log_n(evals.len(), k, points.len());
    let (input, pts) = (scalar_limbs(gpu, evals)?, scalar_limbs(gpu, points)?);
    let mut y = vec![0u64; k * 4];
    check(unsafe { ffi::blsgpu_fr_bary_eval_many(gpu.ctx, input.as_ptr(), log_n, k, pts.as_ptr(), order as c_int, y.as_mut_ptr()) })?;
    limbs_scalars(gpu, &y)
}
/// As `fr_bary_eval`, and the evaluations on the same domain, in the same order, of the quotients (p_v(X) - y_v) / (X - z_v): the
/// scalars of a KZG proof over a Lagrange SRS (`blsgpu_fr_bary_open_many`).  Returns `(y, q)`.
pub fn fr_bary_open(gpu: &Gpu, evals: &[Scalar], k: usize, points: &[Scalar], order: FrOrder) -> Result<(Vec<Scalar>, Vec<Scalar>), Error> {
    if evals.is_empty() && k == 0 { return Ok((Vec::new(), Vec::new())); }
    let log_n = fr_bary_log_n(evals.len(), k, points.len());
    let (input, pts) = (scalar_limbs(gpu, evals)?, scalar_limbs(gpu, points)?);
    let (mut y, mut q) = (vec![0u64; k * 4], vec![0u64; input.len()]);
    check(unsafe {
        ffi::blsgpu_fr_bary_open_many(gpu.ctx, input.as_ptr(), log_n, k, pts.as_ptr(), order as c_int, y.as_mut_ptr(), q.as_mut_ptr())
    })?;
    Ok((limbs_scalars(gpu, &y)?, limbs_scalars(gpu, &q)?))
}
/// A CSR matrix over `Scalar` resident on the GPU (`blsgpu_fr_matrix`): a circuit's constraint matrices, uploaded, validated and planned
/// once and multiplied with every proof's witness.  The FFI layer sees the handle as an untyped pointer; this is its type.
pub struct FrMatrix { handle: *mut c_void, rows: usize, cols: usize }
impl FrMatrix {
    /// `row_ptr` has `n_rows + 1` entries from 0 to `col.len() == val.len()`, non-decreasing; `col[p] < n_cols`.  Columns inside a row may
    /// repeat (they add) and come in any order; rows may be empty.  A malformed matrix is an `Err` naming the first offending row or position.
    pub fn new(gpu: &Gpu, row_ptr: &[u32], col: &[u32], val: &[Scalar], n_cols: usize) -> Result<FrMatrix, Error> {
        assert!(!row_ptr.is_empty() && col.len() == val.len() && *row_ptr.last().unwrap() as usize == col.len());
        let limbs = scalar_limbs(gpu, val)?;
        let mut handle: *mut c_void = std::ptr::null_mut();
        check(unsafe {
            ffi::blsgpu_fr_matrix_upload(gpu.ctx, row_ptr.len() - 1, n_cols, row_ptr.as_ptr(), col.as_ptr(), limbs.as_ptr(),
                                         &mut handle as *mut *mut c_void as *mut c_void)
        })?;
        Ok(FrMatrix { handle, rows: row_ptr.len() - 1, cols: n_cols })
    }
    pub fn rows(&self) -> usize { self.rows }
    pub fn cols(&self) -> usize { self.cols }
    pub fn nnz(&self) -> usize { unsafe { ffi::blsgpu_fr_matrix_nnz(self.handle as *const c_void) } }
}
impl Drop for FrMatrix {
    fn drop(&mut self) { unsafe { ffi::blsgpu_fr_matrix_free(self.handle) } }
}
/// `out[v][i] = sum over row i's entries of val[p] * x[v][col[p]]` for `k = x.len() / m.cols()` right-hand sides laid end to end -- what a
/// caller writes as `a = A z, b = B z, c = C z` row by row; stack A, B and C into one matrix of `3n` rows to apply all three in one call.
pub fn fr_spmv(gpu: &Gpu, m: &FrMatrix, x: &[Scalar]) -> Result<Vec<Scalar>, Error> {
    assert!(m.cols > 0 && x.len() % m.cols == 0);
    let k = x.len() / m.cols;
    if k == 0 || m.rows == 0 { return Ok(Vec::new()); }
    let input = scalar_limbs(gpu, x)?;
    let mut out = vec![0u64; k * m.rows * 4];
    check(unsafe { ffi::blsgpu_fr_spmv(gpu.ctx, m.handle as *const c_void, input.as_ptr(), k, out.as_mut_ptr()) })?;
    limbs_scalars(gpu, &out)
}
/// Binds the TOP variable of `k = tables.len() / 2^m` multilinear tables laid end to end (entry `i` is the value at the point whose
/// coordinate `x_b` is bit `b` of `i`): `out[j][i] = f_j[i] + r * (f_j[i + 2^(m-1)] - f_j[i])`, `k * 2^(m-1)` scalars.
pub fn fr_mle_fold(gpu: &Gpu, tables: &[Scalar], m: u32, r: &Scalar) -> Result<Vec<Scalar>, Error> {
    assert!(m >= 1 && tables.len() % (1usize << m) == 0);
    let k = tables.len() >> m;
    if k == 0 { return Ok(Vec::new()); }
    let (input, rl) = (scalar_limbs(gpu, tables)?, scalar_limbs(gpu, std::slice::from_ref(r))?);
    let mut out = vec![0u64; tables.len() / 2 * 4];
    check(unsafe { ffi::blsgpu_fr_mle_fold(gpu.ctx, input.as_ptr(), m as c_int, k, rl.as_ptr(), out.as_mut_ptr()) })?;
    limbs_scalars(gpu, &out)
}
/// `eq(point)[i] = prod_b (bit b of i ? point[b] : 1 - point[b])`, `2^point.len()` scalars: `f(point) = sum_i f[i] * eq(point)[i]`.
pub fn fr_eq_table(gpu: &Gpu, point: &[Scalar]) -> Result<Vec<Scalar>, Error> {
    let pl = scalar_limbs(gpu, point)?;
    let mut out = vec![0u64; 4usize << point.len()];
    check(unsafe { ffi::blsgpu_fr_eq_table(gpu.ctx, if point.is_empty() { std::ptr::null() } else { pl.as_ptr() }, point.len() as c_int, out.as_mut_ptr()) })?;
    limbs_scalars(gpu, &out)
}
/// `f_j(point)` for `k = tables.len() / 2^point.len()` multilinear tables, `point[b]` the value of `x_b`.
pub fn fr_mle_eval(gpu: &Gpu, tables: &[Scalar], point: &[Scalar]) -> Result<Vec<Scalar>, Error> {
    let m = point.len();
    assert!(tables.len() % (1usize << m) == 0);
    let k = tables.len() >> m;
    if k == 0 { return Ok(Vec::new()); }
    let (input, pl) = (scalar_limbs(gpu, tables)?, scalar_limbs(gpu, point)?);
    let mut out = vec![0u64; k * 4];
    check(unsafe { ffi::blsgpu_fr_mle_eval(gpu.ctx, input.as_ptr(), m as c_int, k, if m == 0 { std::ptr::null() } else { pl.as_ptr() }, out.as_mut_ptr()) })?;
    limbs_scalars(gpu, &out)
}
/// A sumcheck over `sum_x sum_t coef_t * prod_e f_{tables[e]}(x)` resident on the GPU (`blsgpu_fr_sumcheck`): the tables are copied to the
/// device and consumed by the rounds.  The FFI layer sees the handle as an untyped pointer; this is its type.  Order: `round(None)`,
/// `round(Some(&r_1))` ... while `vars_left() > 1`, then `finish(&r_m)`, which returns `f_j` at the point `p_b = r_(m-b)`.
pub struct FrSumcheck<'a> { gpu: &'a Gpu, handle: *mut c_void, k: usize }
impl<'a> FrSumcheck<'a> {
    /// `terms`: (coefficient, table indices) with 1 to 6 indices below `k` each (an index may repeat), at most 8 terms and 8 tables.
    pub fn new(gpu: &'a Gpu, tables: &[Scalar], m: u32, terms: &[(Scalar, Vec<u8>)]) -> Result<FrSumcheck<'a>, Error> {
        assert!(m >= 1 && !tables.is_empty() && tables.len() % (1usize << m) == 0);
        let k = tables.len() >> m;
        let input = scalar_limbs(gpu, tables)?;
        let coef = scalar_limbs(gpu, &terms.iter().map(|t| t.0).collect::<Vec<Scalar>>())?;
        let (mut ptr, mut tab) = (vec![0u32], Vec::<u8>::new());
        for t in terms { tab.extend_from_slice(&t.1); ptr.push(tab.len() as u32); }
        let mut handle: *mut c_void = std::ptr::null_mut();
        check(unsafe {
            ffi::blsgpu_fr_sumcheck_begin(gpu.ctx, input.as_ptr(), m as c_int, k, terms.len(), ptr.as_ptr(), tab.as_ptr(), coef.as_ptr(),
                                          &mut handle as *mut *mut c_void as *mut c_void)
        })?;
        Ok(FrSumcheck { gpu, handle, k })
    }
    pub fn vars_left(&self) -> usize { unsafe { ffi::blsgpu_fr_sumcheck_vars_left(self.handle as *const c_void) as usize } }
    pub fn degree(&self) -> usize { unsafe { ffi::blsgpu_fr_sumcheck_degree(self.handle as *const c_void) as usize } }
    /// The round polynomial's values at `0 ..= degree()`; `r_prev` is `None` in the first round only.
    pub fn round(&mut self, r_prev: Option<&Scalar>) -> Result<Vec<Scalar>, Error> {
        let rl = match r_prev { Some(r) => scalar_limbs(self.gpu, std::slice::from_ref(r))?, None => Vec::new() };
        let mut out = vec![0u64; (self.degree() + 1) * 4];
        check(unsafe { ffi::blsgpu_fr_sumcheck_round(self.gpu.ctx, self.handle, if r_prev.is_some() { rl.as_ptr() } else { std::ptr::null() }, out.as_mut_ptr()) })?;
        limbs_scalars(self.gpu, &out)
    }
    pub fn finish(&mut self, r_last: &Scalar) -> Result<Vec<Scalar>, Error> {
        let rl = scalar_limbs(self.gpu, std::slice::from_ref(r_last))?;
        let mut out = vec![0u64; self.k * 4];
        check(unsafe { ffi::blsgpu_fr_sumcheck_finish(self.gpu.ctx, self.handle, rl.as_ptr(), out.as_mut_ptr()) })?;
        limbs_scalars(self.gpu, &out)
    }
}
impl<'a> Drop for FrSumcheck<'a> {
    fn drop(&mut self) { unsafe { ffi::blsgpu_fr_sumcheck_free(self.handle) } }
}
/// Which partial rounds a `FrPoseidon` runs: `Auto` (a request) derives the sparse form when the matrix allows it.
#[derive(Clone, Copy, PartialEq, Eq, Debug)]
pub enum FrPoseidonForm { Auto = 0, Dense = 1, Sparse = 2 }
/// A Poseidon instance over `Scalar` resident on the GPU (`blsgpu_fr_poseidon`): width `t`, `r_full` full and `r_partial` partial rounds,
/// `(r_full + r_partial) * t` round constants and the `t * t` matrix (row-major).  THE PARAMETERS ARE THE CALLER'S: the library ships no
/// standard set.  Validated and planned once.  The FFI layer sees the handle as an untyped pointer; this is its type.
pub struct FrPoseidon<'a> { gpu: &'a Gpu, handle: *mut c_void }
impl<'a> FrPoseidon<'a> {
    pub fn new(gpu: &'a Gpu, t: usize, r_full: usize, r_partial: usize, round_constants: &[Scalar], mds: &[Scalar], form: FrPoseidonForm) -> Result<FrPoseidon<'a>, Error> {
        assert!(round_constants.len() == (r_full + r_partial) * t && mds.len() == t * t);
        let (rc, mm) = (scalar_limbs(gpu, round_constants)?, scalar_limbs(gpu, mds)?);
        let mut handle: *mut c_void = std::ptr::null_mut();
        check(unsafe {
            ffi::blsgpu_fr_poseidon_create(gpu.ctx, t as c_int, r_full as c_int, r_partial as c_int, rc.as_ptr(), mm.as_ptr(), form as c_int,
                                           &mut handle as *mut *mut c_void as *mut c_void)
        })?;
        Ok(FrPoseidon { gpu, handle })
    }
    pub fn width(&self) -> usize { unsafe { ffi::blsgpu_fr_poseidon_width(self.handle as *const c_void) as usize } }
    pub fn rounds_full(&self) -> usize { unsafe { ffi::blsgpu_fr_poseidon_rounds_full(self.handle as *const c_void) as usize } }
    pub fn rounds_partial(&self) -> usize { unsafe { ffi::blsgpu_fr_poseidon_rounds_partial(self.handle as *const c_void) as usize } }
    /// `Dense` or `Sparse`: what the handle runs.
    pub fn form(&self) -> FrPoseidonForm {
        if unsafe { ffi::blsgpu_fr_poseidon_form(self.handle as *const c_void) } == 2 { FrPoseidonForm::Sparse } else { FrPoseidonForm::Dense }
    }
    pub fn products_per_permutation(&self) -> usize { unsafe { ffi::blsgpu_fr_poseidon_products(self.handle as *const c_void) } }
    /// `states.len() / t` states of `t` scalars laid end to end -> the permuted states.
    pub fn permute(&self, states: &[Scalar]) -> Result<Vec<Scalar>, Error> {
        assert!(states.len() % self.width() == 0);
        if states.is_empty() { return Ok(Vec::new()); }
        let input = scalar_limbs(self.gpu, states)?;
        let mut out = vec![0u64; input.len()];
        check(unsafe { ffi::blsgpu_fr_poseidon_permute(self.gpu.ctx, self.handle as *const c_void, input.as_ptr(), states.len() / self.width(), out.as_mut_ptr()) })?;
        limbs_scalars(self.gpu, &out)
    }
    /// Preimages of `t - 1` scalars -> one digest each: element 1 of the permutation of `(tag, x_1 .. x_(t-1))`.
    pub fn hash_many(&self, tag: &Scalar, inputs: &[Scalar]) -> Result<Vec<Scalar>, Error> {
        let a = self.width() - 1;
        assert!(inputs.len() % a == 0);
        if inputs.is_empty() { return Ok(Vec::new()); }
        let (tg, input) = (scalar_limbs(self.gpu, std::slice::from_ref(tag))?, scalar_limbs(self.gpu, inputs)?);
        let n = inputs.len() / a;
        let mut out = vec![0u64; n * 4];
        check(unsafe { ffi::blsgpu_fr_poseidon_hash_many(self.gpu.ctx, self.handle as *const c_void, tg.as_ptr(), input.as_ptr(), n, out.as_mut_ptr()) })?;
        limbs_scalars(self.gpu, &out)
    }
    /// `k` trees of `(t-1)^height` leaves each, tree after tree -> `(roots, nodes)`: `nodes` holds every inner level, level 1 first and the
    /// roots last.
    pub fn merkle(&self, tag: &Scalar, leaves: &[Scalar], height: u32, k: usize) -> Result<(Vec<Scalar>, Vec<Scalar>), Error> {
        let a = self.width() - 1;
        let per = a.pow(height);
        assert!(leaves.len() == k * per);
        if k == 0 { return Ok((Vec::new(), Vec::new())); }
        let count = if a == 1 { k * height as usize } else { k * ((per - 1) / (a - 1)) };
        let (tg, input) = (scalar_limbs(self.gpu, std::slice::from_ref(tag))?, scalar_limbs(self.gpu, leaves)?);
        let (mut roots, mut nodes) = (vec![0u64; k * 4], vec![0u64; count * 4]);
        check(unsafe {
            ffi::blsgpu_fr_poseidon_merkle(self.gpu.ctx, self.handle as *const c_void, tg.as_ptr(), input.as_ptr(), height as c_int, k,
                                           if count > 0 { nodes.as_mut_ptr() } else { std::ptr::null_mut() }, roots.as_mut_ptr())
        })?;
        Ok((limbs_scalars(self.gpu, &roots)?, limbs_scalars(self.gpu, &nodes)?))
    }
}
impl<'a> Drop for FrPoseidon<'a> {
    fn drop(&mut self) { unsafe { ffi::blsgpu_fr_poseidon_free(self.handle) } }
}
/// An operand of an `FrExpr` instruction (`BLSGPU_FR_EXPR_REG` / `_COL` / `_CONST`).
#[derive(Clone, Copy, PartialEq, Eq, Debug)]
pub enum FrExprOperand { Reg(u8), Col(u8, i16), Const(u8) }
impl FrExprOperand {
    pub fn word(self) -> u32 {
        match self {
            FrExprOperand::Reg(i) => i as u32,
            FrExprOperand::Col(j, rot) => 0x4000_0000 | (((rot as u16) as u32) << 8) | j as u32,
            FrExprOperand::Const(i) => 0x8000_0000 | i as u32,
        }
    }
}
/// One instruction of an `FrExpr`: `Mad` is dst = dst + a * b, `Mov` takes one operand.
#[derive(Clone, Copy, PartialEq, Eq, Debug)]
pub enum FrExprInstr {
    Add(u8, FrExprOperand, FrExprOperand), Sub(u8, FrExprOperand, FrExprOperand), Mul(u8, FrExprOperand, FrExprOperand), Mad(u8, FrExprOperand, FrExprOperand),
    Mov(u8, FrExprOperand),
}
impl FrExprInstr {
    pub fn words(self) -> [u32; 3] {
        let (op, dst, a, b) = match self {
            FrExprInstr::Add(d, a, b) => (0u32, d, a.word(), b.word()), FrExprInstr::Sub(d, a, b) => (1, d, a.word(), b.word()),
            FrExprInstr::Mul(d, a, b) => (2, d, a.word(), b.word()), FrExprInstr::Mad(d, a, b) => (3, d, a.word(), b.word()),
            FrExprInstr::Mov(d, a) => (4, d, a.word(), 0),
        };
        [op | ((dst as u32) << 8), a, b]
    }
}
/// An expression program over `Scalar` columns resident on the GPU (`blsgpu_fr_expr`): straight-line code over columns, registers and
/// constants, validated once by `new` (a bad program is an `Err` naming the instruction and the rule) and evaluated per row in one pass:
/// gate and quotient columns of a PLONK-style prover.  The FFI layer sees the handle as an untyped pointer; this is its type.
pub struct FrExpr<'a> { gpu: &'a Gpu, handle: *mut c_void }
impl<'a> FrExpr<'a> {
    pub fn new(gpu: &'a Gpu, n_cols: usize, n_regs: usize, consts: &[Scalar], code: &[FrExprInstr]) -> Result<FrExpr<'a>, Error> {
        let cs = if consts.is_empty() { Vec::new() } else { scalar_limbs(gpu, consts)? };
        let words: Vec<u32> = code.iter().flat_map(|i| i.words()).collect();
        let mut handle: *mut c_void = std::ptr::null_mut();
        check(unsafe {
            ffi::blsgpu_fr_expr_create(gpu.ctx, n_cols as c_int, n_regs as c_int, consts.len() as c_int, if cs.is_empty() { std::ptr::null() } else { cs.as_ptr() }, code.len(),
                                       words.as_ptr(), &mut handle as *mut *mut c_void as *mut c_void)
        })?;
        Ok(FrExpr { gpu, handle })
    }
    pub fn cols(&self) -> usize { unsafe { ffi::blsgpu_fr_expr_cols(self.handle as *const c_void) as usize } }
    pub fn regs(&self) -> usize { unsafe { ffi::blsgpu_fr_expr_regs(self.handle as *const c_void) as usize } }
    pub fn instructions(&self) -> usize { unsafe { ffi::blsgpu_fr_expr_instructions(self.handle as *const c_void) } }
    pub fn products_per_row(&self) -> usize { unsafe { ffi::blsgpu_fr_expr_products(self.handle as *const c_void) } }
    /// Bit j: some instruction reads column j.
    pub fn cols_read(&self) -> u32 { unsafe { ffi::blsgpu_fr_expr_cols_read(self.handle as *const c_void) as u32 } }
    /// The program over 2^`log_n` rows: column j has `columns[j].len()` scalars, a power of two at most 2^`log_n` (an empty slice for a
    /// column the program does not read), and is read modulo its own length at row + rot * 2^`log_stride`.
    ///
    /// # Panics
    /// If there is not one slice per column or a length is not a power of two at most 2^`log_n` (the C ABI cannot see slice lengths: the
    /// sizes are checked here, before the call).  What the library itself refuses comes back as `Err`.
    pub fn eval(&self, columns: &[&[Scalar]], log_n: u32, log_stride: u32) -> Result<Vec<Scalar>, Error> {
        assert!(columns.len() == self.cols() && log_n <= 28);
        let n = 1usize << log_n;
        let mut limbs: Vec<Vec<u64>> = Vec::with_capacity(columns.len());
        let mut lens = vec![0u8; columns.len()];
        for (j, c) in columns.iter().enumerate() {
            if c.is_empty() { limbs.push(Vec::new()); continue; }
            assert!(c.len().is_power_of_two() && c.len() <= n);
            lens[j] = c.len().trailing_zeros() as u8;
            limbs.push(scalar_limbs(self.gpu, c)?);
        }
        let ptrs: Vec<*const c_void> = limbs.iter().map(|l| if l.is_empty() { std::ptr::null() } else { l.as_ptr() as *const c_void }).collect();
        let mut out = vec![0u64; n * 4];
        check(unsafe {
            ffi::blsgpu_fr_expr_eval(self.gpu.ctx, self.handle as *const c_void, ptrs.as_ptr(), lens.as_ptr(), log_n as c_int, log_stride as c_int, out.as_mut_ptr())
        })?;
        limbs_scalars(self.gpu, &out)
    }
}
impl<'a> Drop for FrExpr<'a> {
    fn drop(&mut self) { unsafe { ffi::blsgpu_fr_expr_free(self.handle) } }
}
/// What `FrLookup::count` returns: the multiplicity column (`rows` scalars), the first table row of every looked-up row
/// (`FrLookup::MISS` for none) and the number of looked-up rows that are in no table row.
pub struct FrLookupCounts { pub mult: Vec<Scalar>, pub index: Vec<u32>, pub missing: u64 }
/// A lookup table over `Scalar` keys resident on the GPU (`blsgpu_fr_lookup`): an index over rows of c scalars, built once; `count` gives
/// the logUp multiplicity column a prover commits to before it draws its challenges (m[j] = how often row j's key is looked up if j is the
/// FIRST row with that key, else 0; r - m with `negate`, ready for the fraction sum's `mult`).  The FFI layer sees the handle as an
/// untyped pointer; this is its type.
pub struct FrLookup<'a> { gpu: &'a Gpu, handle: *mut c_void }
impl<'a> FrLookup<'a> {
    pub const MISS: u32 = 0xFFFF_FFFF;
    /// `columns[j][i]` is scalar j of table row i: c = `columns.len()` in 1..=8 columns of equal length.
    ///
    /// # Panics
    /// If there is no column or the columns differ in length (the C ABI cannot see slice lengths).
    pub fn new(gpu: &'a Gpu, columns: &[&[Scalar]]) -> Result<FrLookup<'a>, Error> {
        let (limbs, rows) = Self::pack(gpu, columns)?;
        let mut handle: *mut c_void = std::ptr::null_mut();
        check(unsafe { ffi::blsgpu_fr_lookup_create(gpu.ctx, columns.len() as c_int, limbs.as_ptr(), rows, &mut handle as *mut *mut c_void as *mut c_void) })?;
        Ok(FrLookup { gpu, handle })
    }
    fn pack(gpu: &Gpu, columns: &[&[Scalar]]) -> Result<(Vec<u64>, usize), Error> {
        assert!(!columns.is_empty() && columns.iter().all(|c| c.len() == columns[0].len()));
        let mut limbs = Vec::with_capacity(columns.len() * columns[0].len() * 4);
        for c in columns { if !c.is_empty() { limbs.extend(scalar_limbs(gpu, c)?); } }
        Ok((limbs, columns[0].len()))
    }
    pub fn cols(&self) -> usize { unsafe { ffi::blsgpu_fr_lookup_cols(self.handle as *const c_void) as usize } }
    pub fn rows(&self) -> usize { unsafe { ffi::blsgpu_fr_lookup_rows(self.handle as *const c_void) } }
    pub fn distinct(&self) -> usize { unsafe { ffi::blsgpu_fr_lookup_distinct(self.handle as *const c_void) } }
    pub fn slots(&self) -> usize { unsafe { ffi::blsgpu_fr_lookup_slots(self.handle as *const c_void) } }
    /// Counts the looked-up rows `f` (one slice per table column, equal lengths; empty slices are a valid, empty lookup).
    ///
    /// # Panics
    /// If there is not one slice per table column or the slices differ in length.
    pub fn count(&self, f: &[&[Scalar]], negate: bool) -> Result<FrLookupCounts, Error> {
        assert!(f.len() == self.cols());
        let (limbs, n) = Self::pack(self.gpu, f)?;
        let mut mult = vec![0u64; self.rows() * 4];
        let mut index = vec![0u32; n];
        let mut missing = 0u64;
        check(unsafe {
            ffi::blsgpu_fr_lookup_count(self.gpu.ctx, self.handle as *const c_void, if n == 0 { std::ptr::null() } else { limbs.as_ptr() }, n, negate as c_int, mult.as_mut_ptr(),
                                        if n == 0 { std::ptr::null_mut() } else { index.as_mut_ptr() }, &mut missing as *mut u64)
        })?;
        Ok(FrLookupCounts { mult: limbs_scalars(self.gpu, &mult)?, index, missing })
    }
}
impl<'a> Drop for FrLookup<'a> {
    fn drop(&mut self) { unsafe { ffi::blsgpu_fr_lookup_free(self.handle) } }
}
fn split72(flat: Vec<u64>) -> Vec<GtLimbs> {
    flat.chunks_exact(72).map(|c| { let mut a = [0u64; 72]; a.copy_from_slice(c); GtLimbs(a) }).collect()
}

/// Batched `pairing` (src/pairings.rs:607-653): out[i] = e(p[i], q[i]); an identity on either side gives Gt::identity().
pub fn pairing_batch(gpu: &Gpu, p: &[G1Affine], q: &[G2Affine]) -> Result<Vec<GtLimbs>, Error> {
    assert_eq!(p.len(), q.len());
    let n = p.len();
    let ((g1, f1), (g2, f2)) = (g1_wire(gpu, p)?, g2_wire(gpu, q)?);
    let mut out = vec![0u64; n * 72];
    check(unsafe { ffi::blsgpu_pairing_batch(gpu.ctx, g1.as_ptr(), f1.as_ptr(), g2.as_ptr(), f2.as_ptr(), n, out.as_mut_ptr()) })?;
    Ok(split72(out))
}

/// `multi_miller_loop` (src/pairings.rs:554-603) over (P_i, Q_i): the raw `MillerLoopResult` limbs.  The reference's
/// `G2Prepared` caches 68 line triples per point (19 584 B); the GPU recomputes the lines from the affine point instead.
pub fn multi_miller_loop(gpu: &Gpu, terms: &[(&G1Affine, &G2Affine)]) -> Result<GtLimbs, Error> {
    let p: Vec<G1Affine> = terms.iter().map(|t| *t.0).collect();
    let q: Vec<G2Affine> = terms.iter().map(|t| *t.1).collect();
    let ((g1, f1), (g2, f2)) = (g1_wire(gpu, &p)?, g2_wire(gpu, &q)?);
    let mut out = [0u64; 72];
    check(unsafe { ffi::blsgpu_multi_miller_loop(gpu.ctx, g1.as_ptr(), f1.as_ptr(), g2.as_ptr(), f2.as_ptr(), terms.len(), out.as_mut_ptr()) })?;
    Ok(GtLimbs(out))
}

/// `G2Prepared` values resident on the device (src/pairings.rs:487-546: the 68 line-coefficient triples of FIXED G2 arguments, computed
/// once by `blsgpu_g2_prepare`); the prepared Miller loops name them by index.
pub struct PreparedG2<'a> { gpu: &'a Gpu, handle: *mut ffi::BlsgpuG2Prepared, len: usize }
impl<'a> PreparedG2<'a> {
    pub fn new(gpu: &'a Gpu, points: &[G2Affine]) -> Result<Self, Error> {
        let (g2, f2) = g2_wire(gpu, points)?;
        let mut handle = core::ptr::null_mut();
        check(unsafe { ffi::blsgpu_g2_prepare(gpu.ctx, g2.as_ptr(), f2.as_ptr(), points.len(), &mut handle) })?;
        Ok(PreparedG2 { gpu, handle, len: points.len() })
    }
    pub fn len(&self) -> usize { self.len }
    pub fn is_empty(&self) -> bool { self.len == 0 }
    /// `multi_miller_loop` over terms (P_i, Q_i) with Q_i = table[i_q] (`Ok(index)`) or a fresh point (`Err(&G2Affine)`, lines on the fly)
    pub fn multi_miller_loop(&self, terms: &[(&G1Affine, Result<u32, &G2Affine>)]) -> Result<GtLimbs, Error> {
        let p: Vec<G1Affine> = terms.iter().map(|t| *t.0).collect();
        let q: Vec<G2Affine> = terms.iter().map(|t| match t.1 { Ok(_) => G2Affine::identity(), Err(q) => *q }).collect();
        let qi: Vec<u32> = terms.iter().map(|t| match t.1 { Ok(i) => i, Err(_) => u32::MAX }).collect();
        let ((g1, f1), (g2, f2)) = (g1_wire(self.gpu, &p)?, g2_wire(self.gpu, &q)?);
        let mut out = [0u64; 72];
        check(unsafe { ffi::blsgpu_multi_miller_loop_prepared(self.gpu.ctx, g1.as_ptr(), f1.as_ptr(), g2.as_ptr(), f2.as_ptr(), qi.as_ptr(), self.handle, terms.len(), out.as_mut_ptr()) })?;
        Ok(GtLimbs(out))
    }
}
impl Drop for PreparedG2<'_> { fn drop(&mut self) { unsafe { ffi::blsgpu_g2_prepared_free(self.handle) } } }

/// N independent `multi_miller_loop(terms).final_exponentiation()` in ONE device call (bulk signature verification: one product of
/// k pairings per equation, src/pairings.rs:554-603, 817-824, 48-176): the `Gt` limbs of every equation; `final_exp = false` returns
/// the raw `MillerLoopResult` limbs.  An equation without terms gives `Gt::identity()` / `MillerLoopResult::default()`.
pub fn multi_miller_loop_many(gpu: &Gpu, equations: &[&[(&G1Affine, &G2Affine)]], final_exp: bool) -> Result<Vec<GtLimbs>, Error> {
    let p: Vec<G1Affine> = equations.iter().flat_map(|e| e.iter().map(|t| *t.0)).collect();
    let q: Vec<G2Affine> = equations.iter().flat_map(|e| e.iter().map(|t| *t.1)).collect();
    let mut off = Vec::with_capacity(equations.len() + 1);
    off.push(0u64);
    for e in equations { off.push(off[off.len() - 1] + e.len() as u64); }
    let ((g1, f1), (g2, f2)) = (g1_wire(gpu, &p)?, g2_wire(gpu, &q)?);
    let mut out = vec![0u64; equations.len() * 72];
    check(unsafe { ffi::blsgpu_multi_miller_loop_many(gpu.ctx, g1.as_ptr(), f1.as_ptr(), g2.as_ptr(), f2.as_ptr(), off.as_ptr(), equations.len(), final_exp as c_int, out.as_mut_ptr()) })?;
    Ok(split72(out))
}

/// `MillerLoopResult::final_exponentiation` (src/pairings.rs:48-176) for a batch of raw Miller values.
pub fn final_exponentiation(gpu: &Gpu, f: &[GtLimbs]) -> Result<Vec<GtLimbs>, Error> {
    let flat: Vec<u64> = f.iter().flat_map(|g| g.0).collect();
    let mut out = vec![0u64; flat.len()];
    check(unsafe { ffi::blsgpu_final_exponentiation_batch(gpu.ctx, flat.as_ptr(), f.len(), out.as_mut_ptr()) })?;
    Ok(split72(out))
}

/// `MillerLoopResult + MillerLoopResult` / `Gt + Gt` folded over a slice (src/pairings.rs:179-186): how partial products of a
/// sharded `multi_miller_loop` are combined before the single final exponentiation.
pub fn fp12_product(gpu: &Gpu, f: &[GtLimbs]) -> Result<GtLimbs, Error> {
    let flat: Vec<u64> = f.iter().flat_map(|g| g.0).collect();
    let mut out = [0u64; 72];
    check(unsafe { ffi::blsgpu_fp12_product(gpu.ctx, flat.as_ptr(), f.len(), out.as_mut_ptr()) })?;
    Ok(GtLimbs(out))
}

/// `&Gt * &Scalar` (src/pairings.rs:297-322) for n pairs.
pub fn gt_mul_scalar(gpu: &Gpu, gt: &[GtLimbs], scalars: &[Scalar]) -> Result<Vec<GtLimbs>, Error> {
    assert_eq!(gt.len(), scalars.len());
    let flat: Vec<u64> = gt.iter().flat_map(|g| g.0).collect();
    let s = scalar_bytes(scalars);
    let mut out = vec![0u64; flat.len()];
    check(unsafe { ffi::blsgpu_gt_mul_scalar_batch(gpu.ctx, flat.as_ptr(), s.as_ptr(), gt.len(), out.as_mut_ptr()) })?;
    Ok(split72(out))
}

/// `G1Projective::batch_normalize` (src/g1.rs:806-839).  Out of tree the projective limbs are not reachable, so the points
/// travel as affine encodings already; this wrapper exists for symmetry and simply maps `to_affine` (`Curve::to_affine`).
/// The limb-level version (Montgomery's trick on the GPU, `blsgpu_g1_batch_normalize`) is in `in-tree/hip.rs`.
pub fn batch_normalize_g1(points: &[G1Projective]) -> Vec<G1Affine> {
    let mut out = vec![G1Affine::identity(); points.len()];
    G1Projective::batch_normalize(points, &mut out);
    out
}

/// Resident bases (e.g. an SRS): uploaded once, reused by any number of MSMs (`blsgpu_g1_bases_upload`, `blsgpu_g1_msm`).
pub struct ResidentG1<'a> { gpu: &'a Gpu, handle: *mut ffi::BlsgpuBases, len: usize }
impl<'a> ResidentG1<'a> {
    pub fn upload(gpu: &'a Gpu, bases: &[G1Affine]) -> Result<Self, Error> {
        let (xy, inf) = g1_wire(gpu, bases)?;
        let mut handle = core::ptr::null_mut();
        check(unsafe { ffi::blsgpu_g1_bases_upload(gpu.ctx, xy.as_ptr(), inf.as_ptr(), bases.len(), &mut handle) })?;
        Ok(ResidentG1 { gpu, handle, len: bases.len() })
    }
    pub fn len(&self) -> usize { self.len }
    pub fn is_empty(&self) -> bool { self.len == 0 }
    /// sum_i scalars[i] * bases[first + i]; the result comes back as projective wire limbs and is normalised on the GPU
    pub fn msm(&self, first: usize, scalars: &[Scalar]) -> Result<G1Projective, Error> {
        let s = scalar_bytes(scalars);
        let mut xyz = [0u64; 18];
        check(unsafe { ffi::blsgpu_g1_msm(self.gpu.ctx, self.handle, first, s.as_ptr(), scalars.len(), xyz.as_mut_ptr()) })?;
        let (mut xy, mut inf, mut enc) = ([0u64; 12], [0u8; 1], [0u8; 96]);
        check(unsafe { ffi::blsgpu_g1_batch_normalize(self.gpu.ctx, xyz.as_ptr(), 1, xy.as_mut_ptr(), inf.as_mut_ptr()) })?;
        check(unsafe { ffi::blsgpu_g1_to_bytes_batch(self.gpu.ctx, xy.as_ptr(), inf.as_ptr(), 1, 0, enc.as_mut_ptr()) })?;
        let aff = Option::<G1Affine>::from(G1Affine::from_uncompressed_unchecked(&enc)).expect("libblsgpu returned an invalid G1 encoding");
        Ok(G1Projective::from(aff))
    }
}
impl Drop for ResidentG1<'_> { fn drop(&mut self) { unsafe { ffi::blsgpu_bases_free(self.handle) } } }

/// Every listed GPU of the node behind one handle (`blsgpu_group_*`): MSMs, batches of pairings and `multi_miller_loop`s are dealt to
/// the members in contiguous slices -- one context and one host thread per member inside the library -- and the members' partial results
/// (one group element each) are folded with the reference's own operators, `Sum` (src/g1.rs:161-171) and `MillerLoopResult +
/// MillerLoopResult` (src/pairings.rs:179-186), followed by ONE final exponentiation.  The decoders run on member 0's context.
pub struct GpuGroup { group: *mut ffi::BlsgpuGroup, first: Gpu }
unsafe impl Send for GpuGroup {}
impl Drop for GpuGroup { fn drop(&mut self) { unsafe { ffi::blsgpu_group_destroy(self.group) } } }
impl GpuGroup {
    pub fn new(devices: &[i32]) -> Result<GpuGroup, Error> {
        let mut group = core::ptr::null_mut();
        check(unsafe { ffi::blsgpu_group_create(devices.as_ptr(), devices.len() as c_int, &mut group) })?;
        // a context of its own for the byte decoders (the members' contexts belong to the group's worker threads during a call)
        match Gpu::new(devices[0]) {
            Ok(first) => Ok(GpuGroup { group, first }),
            Err(e) => { unsafe { ffi::blsgpu_group_destroy(group) }; Err(e) }
        }
    }
    pub fn all_devices() -> Result<GpuGroup, Error> {
        let d: Vec<i32> = (0..Gpu::device_count().max(1)).collect();
        GpuGroup::new(&d)
    }
    pub fn len(&self) -> usize { unsafe { ffi::blsgpu_group_size(self.group) as usize } }
    pub fn is_empty(&self) -> bool { self.len() == 0 }
    /// `bases.iter().zip(scalars).map(|(p, s)| p * s).sum::<G1Projective>()` sharded over the members
    pub fn msm_g1(&self, bases: &[G1Affine], scalars: &[Scalar]) -> Result<G1Projective, Error> {
        assert_eq!(bases.len(), scalars.len());
        let ((xy, inf), s) = (g1_wire(&self.first, bases)?, scalar_bytes(scalars));
        let mut gb = core::ptr::null_mut();
        check(unsafe { ffi::blsgpu_group_bases_upload(self.group, 1, xy.as_ptr(), inf.as_ptr(), bases.len(), &mut gb) })?;
        let mut xyz = [0u64; 18];
        let rc = unsafe { ffi::blsgpu_g1_msm_sharded(self.group, gb, s.as_ptr(), bases.len(), xyz.as_mut_ptr()) };
        unsafe { ffi::blsgpu_group_bases_free(gb) };
        check(rc)?;
        let (mut axy, mut ainf, mut enc) = ([0u64; 12], [0u8; 1], [0u8; 96]);
        check(unsafe { ffi::blsgpu_g1_batch_normalize(self.first.ctx, xyz.as_ptr(), 1, axy.as_mut_ptr(), ainf.as_mut_ptr()) })?;
        check(unsafe { ffi::blsgpu_g1_to_bytes_batch(self.first.ctx, axy.as_ptr(), ainf.as_ptr(), 1, 0, enc.as_mut_ptr()) })?;
        Ok(G1Projective::from(Option::<G1Affine>::from(G1Affine::from_uncompressed_unchecked(&enc)).expect("libblsgpu returned an invalid G1 encoding")))
    }
    /// out[i] = e(p[i], q[i]), index slices per member
    pub fn pairing_batch(&self, p: &[G1Affine], q: &[G2Affine]) -> Result<Vec<GtLimbs>, Error> {
        assert_eq!(p.len(), q.len());
        let ((g1, f1), (g2, f2)) = (g1_wire(&self.first, p)?, g2_wire(&self.first, q)?);
        let mut out = vec![0u64; p.len() * 72];
        check(unsafe { ffi::blsgpu_pairing_batch_sharded(self.group, g1.as_ptr(), f1.as_ptr(), g2.as_ptr(), f2.as_ptr(), p.len(), out.as_mut_ptr()) })?;
        Ok(split72(out))
    }
    /// `multi_miller_loop(terms).final_exponentiation()`: member-local products, one fold, ONE final exponentiation
    pub fn multi_miller_loop_final_exp(&self, terms: &[(&G1Affine, &G2Affine)]) -> Result<GtLimbs, Error> {
        let p: Vec<G1Affine> = terms.iter().map(|t| *t.0).collect();
        let q: Vec<G2Affine> = terms.iter().map(|t| *t.1).collect();
        let ((g1, f1), (g2, f2)) = (g1_wire(&self.first, &p)?, g2_wire(&self.first, &q)?);
        let mut out = [0u64; 72];
        check(unsafe { ffi::blsgpu_multi_miller_loop_sharded(self.group, g1.as_ptr(), f1.as_ptr(), g2.as_ptr(), f2.as_ptr(), terms.len(), 1, out.as_mut_ptr()) })?;
        Ok(GtLimbs(out))
    }
}

/// `Curve::to_affine` convenience for callers that want affine results.
pub fn to_affine_g1(p: &G1Projective) -> G1Affine { p.to_affine() }
