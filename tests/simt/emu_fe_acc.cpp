// tests/simt/emu_fe_acc.cpp -- the three inlined field products of the G1 bucket accumulation (fe.hip.h mul_inl / sqr_inl / sop2_inl)
// compiled for the HOST (test infrastructure only), in the operand types xyzz_add_mixed_inl (curve.hip.h) instantiates them with and
// in both orders of the column sums (SEQ, see mac() in fe.hip.h), so that the CPU suite can compare them with Python integers at the
// extremes those types allow (tests/test_msm_acc_products.py).  No cross-lane operation: the entry points run in the calling thread.
#define EMU_LANES 4
#include "emu_harness.h"

#include "curve.hip.h"

using namespace bls;

namespace {

template <int A, int V> Fe<A, V> ld(const u32* w) {
  Fe<A, V> r;
  for (int i = 0; i < NL; i++) r.l[i] = w[i];
  return r;
}
template <class T> void st(u32* w, const T& a) {
  for (int i = 0; i < NL; i++) w[i] = a.l[i];
}

// the operand types of xyzz_add_mixed_inl: stored coordinates fe = Fe<1, 12>, the affine x fe1, the sign-adjusted affine y Fe<2, 2>
// (msm.hip.h cond_neg), P / R = sub(Fe<1, 2>, fe) = Fe<3, 15>, PP / PPP / Q = Fe<1, 2>, Q - X3 = sub(Fe<1, 2>, Fe<1, 9>) = Fe<3, 12>,
// -Y1 = neg(fe) = Fe<2, 13>
template <bool SEQ> int product(int kind, const u32* o, u32* out) {
  switch (kind) {
    case 0: st(out, mul_inl<SEQ>(ld<1, 1>(o), ld<1, 12>(o + NL))); return 0;       // U2 = qx ZZ
    case 1: st(out, mul_inl<SEQ>(ld<2, 2>(o), ld<1, 12>(o + NL))); return 0;       // S2 = qy ZZZ
    case 2: st(out, mul_inl<SEQ>(ld<3, 15>(o), ld<1, 2>(o + NL))); return 0;       // PPP = P PP
    case 3: st(out, mul_inl<SEQ>(ld<1, 12>(o), ld<1, 2>(o + NL))); return 0;       // Q = X1 PP, ZZ3, ZZZ3
    case 4: st(out, sqr_inl<SEQ>(ld<3, 15>(o))); return 0;                         // PP = P^2, R^2
    case 5: st(out, sop2_inl<SEQ>(ld<3, 15>(o), ld<3, 12>(o + NL), ld<2, 13>(o + 2 * NL), ld<1, 2>(o + 3 * NL))); return 0;   // Y3
  }
  return -1;
}

}  // namespace

extern "C" {

// ops: n x 4 x 14 limbs (the operands a product does not take are ignored), out: n x 14 limbs
int emu_fe_acc_products(int kind, int seq, const u32* ops, u32* out, size_t n) {
  for (size_t i = 0; i < n; i++) {
    const int rc = seq ? product<true>(kind, ops + i * 4 * NL, out + i * NL) : product<false>(kind, ops + i * 4 * NL, out + i * NL);
    if (rc) return rc;
  }
  return 0;
}
}
