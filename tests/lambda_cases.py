"""The lambda_q16 values at which the MV cost wraps or peaks, shared by the CPU and GPU tests of them (tests/test_oracle_vs_ref.py, the
*_cpu.py tests of the select models, tests/test_gpu_lambda_edges.py).  Every cost the engine reports is distortion + getCost(bits), and
getCost is HM's (lambda_q16 * bits) >> 16 with the product wrapping in 32 bits (TComRdCost.h:172-189).  Plain Python integers here."""
import math

ALL_ONES = 0xFFFFFFFF     # (2^32 - n) >> 16 = 65535 for every bit count 2 <= n <= 65536: the MV cost constant and at its maximum
HALF = 0x80000000         # 32768 for odd n, 0 for even n.  An MV's bit count is the sum of two odd exp-Golomb lengths, hence even: the MV cost
                          # of a search or a refinement is 0 here; the decisions, which add the caller's bits, see both values
WRAP24 = 178956971        # ceil(2^32 / 24): the first wrap at 24 bits, so inside a window some candidates wrap and some do not
BELOW_ONE = 65535         # getCost(n) = n - 1
ABOVE_ONE = 65537         # getCost(n) = n
TINY = 1                  # lambda non-zero, every MV cost 0

LAMBDA_Q16 = (ALL_ONES, HALF, WRAP24, BELOW_ONE, ABOVE_ONE, TINY)
PEAKS = (ALL_ONES, HALF)
WRAPPING = (ALL_ONES, HALF, WRAP24)
ROUNDING = (WRAP24, BELOW_ONE, ABOVE_ONE, TINY)
MAX_MV_COST = 65535       # (x mod 2^32) >> 16


def component_bits(v):
    """TComRdCost::xGetComponentBits: the exp-Golomb length of one MV difference"""
    t = ((-v) << 1) + 1 if v <= 0 else v << 1
    return 2 * (t.bit_length() - 1) + 1


def mv_bits(vx_q, vy_q, pred_x, pred_y):
    """HM's getBits of a quarter-pel MV against a quarter-pel predictor"""
    return component_bits(int(vx_q) - int(pred_x)) + component_bits(int(vy_q) - int(pred_y))


def get_cost(lambda_q16, bits):
    """TComRdCost::getCost: the product wraps in 32 bits"""
    return ((int(lambda_q16) * int(bits)) & 0xFFFFFFFF) >> 16


def get_cost_64(lambda_q16, bits):
    """what a 64-bit product would give: equal to get_cost exactly where the product does not wrap"""
    return (int(lambda_q16) * int(bits)) >> 16


def wraps(lambda_q16, bits):
    return int(lambda_q16) * int(bits) >= 1 << 32


def as_double(lambda_q16):
    """a lambda that hmme_set_lambda / the reference's setLambda turn into lambda_q16 = floor(65536 * sqrt(lambda))"""
    q = int(lambda_q16)
    lam = {ALL_ONES: 4294967295.0, HALF: float(1 << 30)}.get(q, ((q + 0.5) / 65536.0) ** 2)
    assert int(math.floor(65536.0 * math.sqrt(lam))) == q, q
    return lam


assert WRAP24 == -(-(1 << 32) // 24) and wraps(WRAP24, 24) and not wraps(WRAP24, 23)
assert all(get_cost(ALL_ONES, n) == MAX_MV_COST for n in range(2, 200)) and [get_cost(HALF, n) for n in (2, 3, 4, 5)] == [0, 32768, 0, 32768]
assert all(get_cost(BELOW_ONE, n) == n - 1 and get_cost(ABOVE_ONE, n) == n and get_cost(TINY, n) == 0 for n in range(2, 200))
