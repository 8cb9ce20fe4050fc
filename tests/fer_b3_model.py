"""Lane-level model of pt29r_add_b3 / pt29r_from_iso (csrc/fe29r.h) in the style of tests/fer_model.py, which it builds on:
the complete addition (Renes-Costello-Batina, Algorithm 7, a = 0) on y^2 = x^3 + b whose b3 = 3 b is a FIELD ELEMENT held in a
register - the curve a key set's table entries live on, y^2 = x^3 + 7 W^6 with b3 = 21 W^6 per key - and the map back to
secp256k1.  The device code is a transcription of these functions (same names); every width it relies on is asserted inside
fer_model's products, so running the model at the top of the lazy bounds is the overflow proof of the schedule."""
import fer_model as F

ZERO = [0] * F.LANES
K_ADD_T3 = F.lane_const(lambda j, r: (3, 1, 1, 1)[r])


def ptr_add_b3(P1, P2, b3):
    """P1 + P2 on y^2 = x^3 + b3 / 3, complete.  In: X, Z one unit, Y up to two, b3 one unit (all rows); out: all one unit.
    As fer_model.ptr_add with the two multiplications by 21 replaced by row products: b3 t2 in row 3 of the second layer
    (idle in ptr_add), b3 y3' in a layer of its own."""
    X1, Y1, Z1 = P1
    X2, Y2, Z2 = P2
    Y1, Y2 = F.fer_norm(Y1), F.fer_norm(Y2)
    T = F.fer_mul(F.sel((X1, Y1, Z1, Z1)), F.sel((X2, Y2, Z2, Z2)))            # t0 | t1 | t2 | t2
    t0, t1, t2, _ = F.bcast_rows(T)
    e = F.fer_negate(F.fer_add(F.sel((t0, t1, t0, t0)), F.sel((t1, t2, t2, t2))), 2)
    A = F.fer_add(F.sel((X1, Y1, X1, X1)), F.sel((Y1, Z1, Z1, Z1)))
    B = F.fer_add(F.sel((X2, Y2, X2, X2)), F.sel((Y2, Z2, Z2, Z2)))
    U = F.fer_mulsum([(F.sel((A, A, A, b3)), F.sel((B, B, B, t2)))], addend=F.sel((e, e, e, ZERO)))   # t3 | t4 | y3' | b3 t2
    Ts = F.fer_small_norm(T, K_ADD_T3)                                          # 3 t0 | t1 | - | -
    Y = F.fer_mul(U, b3)                                                        # - | - | b3 y3' | -
    t0p, t1n, _, _ = F.bcast_rows(Ts)
    t3, t4, y3, t2p = F.bcast_rows(F.sel((U, U, Y, U)))
    V = F.fer_add(t1n, F.fer_negate(t2p, 1))                                    # t1 - t2'  [3]
    Wp = F.fer_add(t1n, t2p)                                                    # t1 + t2'  [2]
    # X3 = t3 V - t4 y3 | Z3 = t4 W + t3 t0' | Y3 = W V + y3 t0'
    R = F.fer_mulsum([(F.sel((t3, t4, Wp, Wp)), F.sel((V, Wp, V, V))), (F.sel((F.fer_negate(t4, 1), t3, y3, y3)), F.sel((y3, t0p, t0p, t0p)))])
    X3, Z3, Y3, _ = F.bcast_rows(R)
    return X3, Y3, Z3


def iso_consts(w):
    """W (one unit, all rows) -> W, W^3, b3 = 21 W^6 as the kernels form them once per signature (small_call.hip: row_iso_of)"""
    w3 = F.fer_mul(F.fer_mul(w, w), w)
    b3 = F.fer_small_norm(F.fer_mul(w3, w3), F.lane_const(lambda j, r: 21))
    return w, w3, b3


def ptr_from_iso(Pt, w, w3):
    """(X : Y : Z) on y^2 = x^3 + 7 W^6 -> (X W : Y : Z W^3) on secp256k1 (the inverse of (x W^2, y W^3)), one layer"""
    X, Y, Z = Pt
    Mv = F.fer_mul(F.sel((X, X, Z, Z)), F.sel((w, w, w3, w3)))                  # X W | X W | Z W^3 | Z W^3
    X3, Z3 = F.permlane32_swap(Mv, Mv)
    return X3, Y, Z3
