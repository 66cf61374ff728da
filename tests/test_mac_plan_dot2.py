"""Exact-integer check of the carry-capture plan of the two-term Montgomery dot product (rabe_amd/csrc/bn254/fp.h: mont_dot2_raw,
generated for the device as mont_dot2_fp) -- the companion of tests/test_mac_plan.py for a column that carries the products of TWO
a*b terms: up to 16 of them, up to four with a top limb.

The plan comes from the header the kernels compile from (tests/hostsim/fp_dot2.cpp prints it).  With Python integers and worst-case
limbs, the largest value the 64-bit column can hold before every product that issues WITHOUT a capture stays below 2^64, for any
operands below the modulus; and the value that enters the final conditional subtraction is below twice the modulus.  No GPU needed."""
import importlib.util
import os

import pytest

from oracle import bn254 as bn
from tests import dot2_host as dh

W = dh.W
FULL = (1 << 64) - 1
ROOT = dh.ROOT


def limbs(x):
    return [(x >> (32 * i)) & W for i in range(8)]


def top_products(k):
    lo, hi = (0, k) if k < 8 else (k - 7, 7)
    return [i for i in range(lo, hi + 1) if k >= 7 and (i == 7 or k - i == 7)]


def generator():
    spec = importlib.util.spec_from_file_location("gen_fp_asm", os.path.join(ROOT, "tools", "gen_fp_asm.py"))
    gen = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(gen)
    return gen


def first_overflow(mod, safe, last):
    """walks the 16 columns of mont_dot2 in issue order with every limb at its largest; returns None, or (column, product) of the first
    uncaptured product that could leave the 64-bit accumulator.  Also returns how many products skip the capture."""
    p = limbs(mod)
    top = (mod - 1) >> 224                                   # largest top limb of an operand < mod
    incoming, n_uncaptured = 0, 0
    for k in range(16):
        lo, hi = (0, k) if k < 8 else (k - 7, 7)
        tops = top_products(k)
        acc = incoming
        for i in tops:                                        # top-limb products of BOTH terms first, uncaptured
            for _term in range(2):
                acc += top * top if (i == 7 and k - i == 7) else top * W
                if acc > FULL:
                    return (k, "a%d b%d" % (i, k - i)), n_uncaptured
                n_uncaptured += 1
        banked = 0
        for i in range(lo, hi + 1):
            if not (k < 8 and i == k) and (safe[k] >> i) & 1:
                acc += W * p[k - i]
                if acc > FULL:
                    return (k, "m%d p%d" % (i, k - i)), n_uncaptured
                n_uncaptured += 1
        for i in range(lo, hi + 1):
            if i not in tops:
                acc += 2 * W * W; banked += 2
        for i in range(lo, hi + 1):
            if not (k < 8 and i == k) and not (safe[k] >> i) & 1:
                acc += W * p[k - i]; banked += 1
        if k < 8:
            acc += W * p[0]
            if (last >> k) & 1:
                assert banked == 0, "the closing product may skip the capture only in a column without banked products"
                if acc > FULL:
                    return (k, "closing"), n_uncaptured
                n_uncaptured += 1
        incoming = acc >> 32                                  # high word + banked carries of the true (unbounded) sum
        assert incoming < 1 << 37                             # what ColumnPlan's slack of 2^8 units covers, with room
        assert banked < 1 << 32                               # the carry word itself
    return None, n_uncaptured


@pytest.mark.parametrize("field", ["fp", "fr"])
def test_dot2_plan_never_overflows(field):
    mod = dh.MODS[field]
    safe, last = dh.plan(field)
    bad, n_uncaptured = first_overflow(mod, safe, last)
    assert bad is None
    # the plan still saves something: 30 top-limb products and the 19 reduction products it keeps
    assert n_uncaptured >= 30 + 16


@pytest.mark.parametrize("field", ["fp", "fr"])
def test_the_single_product_plan_would_overflow_here(field):
    """the check bites: mont_mul's plan (budgeted for TWO top-limb products per column) is refused for the dot product's columns"""
    mod = dh.MODS[field]
    gen = generator()
    top = limbs(mod)[7] + 1
    safe1, last1 = gen.column_plan(limbs(mod), True, top, top, 1)
    bad, _n = first_overflow(mod, safe1, last1)
    assert bad is not None and bad[0] in (7, 8, 9)
    safe2, last2 = dh.plan(field)
    assert (safe1, last1) != (safe2, last2)
    assert all(s2 & ~s1 == 0 for s1, s2 in zip(safe1, safe2))      # the dot product's safe set is a subset, column by column


@pytest.mark.parametrize("field", ["fp", "fr"])
def test_value_before_the_conditional_subtraction_is_below_twice_the_modulus(field):
    """REDC of T = a0 b0 + a1 b1 <= 2 (mod - 1)^2 adds m * mod with m < 2^256 and divides by 2^256 exactly"""
    mod = dh.MODS[field]
    R = 1 << 256
    t_max = 2 * (mod - 1) ** 2
    assert t_max < mod * R                                     # the issue's bound: the sum is a valid REDC input
    out_max = (t_max + (R - 1) * mod) // R
    assert out_max < 2 * mod < 1 << 255                        # one conditional subtraction, and no ninth word
    assert t_max + (R - 1) * mod < 1 << 512                    # nothing leaves the 16 columns


def test_generated_routine_is_laid_out_for_this_plan():
    """tools/gen_fp_asm.py recomputes the plan with ColumnPlan's rule and ties it to the header with static_asserts"""
    gen = generator()
    mod = gen.fp_mod()
    safe, last = dh.plan("fp")
    assert gen.column_plan(mod, True, mod[7] + 1, mod[7] + 1, 2) == (safe, last)
    text = open(os.path.join(ROOT, "rabe_amd", "csrc", "bn254", "fp_gfx950_gen.h")).read()
    check = text[text.index("namespace gen_check_dot2 {"):]
    check = check[:check.index("}")]
    assert "ColumnPlan<FpParams> plan(true, FpParams::mod(7) + 1, FpParams::mod(7) + 1, 2);" in check
    assert all("plan.safe[%d] == 0x%x" % (k, safe[k]) in check for k in range(16))
    assert "plan.last_safe == 0x%x" % last in check
    # and the routine's instruction counts are what the plan says: 128 a*b + 64 m*p multiply-adds, one capture per banked product
    body = text[text.index("RB_HD void mont_dot2_fp("):]
    body = body[:body.index("cond_sub_mod<FpParams>(r, 0);")]
    n_mad, n_cap = body.count("v_mad_u64_u32"), body.count("v_addc_co_u32_e64")
    n_safe_mp = sum(bin(s).count("1") for s in safe) + bin(last).count("1")
    assert n_mad == 128 + 64
    assert n_cap == n_mad - 30 - n_safe_mp
