"""hipref.check_sched -- the host invariant every scheduling test of tests/test_gpu_sched.py checks between
set_weights and submit -- on hand-written hand-outs: it must accept what the kernels can decode and reject,
naming the field, what they cannot.  No GPU, no library call."""
import pytest

import cases as C
import hipref


def _sched(**kw):
    s = dict(th=2, tw=56, linear=1, uy=28, ux=1, total_units=0, half_from=0x7fffffff, static_rounds=2, lazy_queue=0,
             pool=0, teams=512, roles=0, ring_waits=0)
    s.update(kw)
    return s


# N = 64, 112x112, 32 -> 32 -> 512, u8: 4-row units, 28 per image, 1792 in all
ROLES_112 = C.ConvCase("r112", 64, 32, 112, 112, 32, 512, dst_dt=C.U8)
# N = 80, 56x56, 64 -> 64 -> 256, s32 (conv_mfma.cuh's kernel): 2-row units, 28 per image, 2240 in all
FUSED_56 = C.ConvCase("f56", 80, 64, 56, 56, 64, 256, dst_dt=C.S32)


def test_accepts_plain_op():
    hipref.check_sched(ROLES_112, _sched(th=4, tw=112, uy=28, total_units=1792, lazy_queue=1, roles=1))
    hipref.check_sched(FUSED_56, _sched(th=4, uy=14, total_units=1120, static_rounds=3))
    # column-split units, fused pooling, the namedtuple form
    hipref.check_sched(FUSED_56, hipref.dfa.ConvSched(th=4, tw=32, linear=0, uy=14, ux=2, total_units=2240, half_from=0x7fffffff,
                                                static_rounds=3, lazy_queue=0, pool=1, teams=512, roles=0, ring_waits=3))


def test_accepts_fused_kernel_op_with_halves():
    # 2240 units, the last 77 handed out as 154 halves
    hipref.check_sched(FUSED_56, _sched(th=2, uy=28, total_units=2240 + 77, half_from=2240 - 77, lazy_queue=1))
    # the clamp reached exactly: nh = units - (static_rounds + 1) * teams = 1792 - 1536
    hipref.check_sched(ROLES_112, _sched(th=4, tw=112, uy=28, total_units=2048, half_from=1536, lazy_queue=1))


def _rejected(case, s, field):
    with pytest.raises(AssertionError) as e:
        hipref.check_sched(case, s)
    assert str(e.value).startswith(field + ":"), str(e.value)
    return str(e.value)


def test_rejects_halves_on_the_role_specialised_kernel():
    """the state of the 112x112 op before half units were confined to conv_mfma.cuh: 1792 units, ids 1792..2047
    would have been decoded as whole units of images 64..73"""
    msg = _rejected(ROLES_112, _sched(th=4, tw=112, uy=28, total_units=2048, half_from=1536, lazy_queue=1, roles=1), "roles")
    assert "1536..2047 of 1792" in msg


def test_rejects_halves_of_an_odd_unit_height():
    _rejected(C.ConvCase("odd", 80, 64, 57, 56, 64, 256, dst_dt=C.S32),
              _sched(th=3, uy=19, total_units=1520 + 77, half_from=1520 - 77, lazy_queue=1), "th")


def test_rejects_halves_with_fused_pooling():
    _rejected(FUSED_56, _sched(th=2, uy=28, total_units=2240 + 77, half_from=2240 - 77, lazy_queue=1, pool=1), "pool")


def test_rejects_halves_without_lazy_draws():
    _rejected(FUSED_56, _sched(th=2, uy=28, total_units=2240 + 77, half_from=2240 - 77, lazy_queue=0), "lazy_queue")


def test_rejects_total_units_off_by_one():
    _rejected(FUSED_56, _sched(th=2, uy=28, total_units=2241), "total_units")
    _rejected(FUSED_56, _sched(th=2, uy=28, total_units=2239), "total_units")
    # with halves: one id more than 2 * nh halves need
    _rejected(FUSED_56, _sched(th=2, uy=28, total_units=2240 + 78, half_from=2240 - 77, lazy_queue=1), "half_from")
    _rejected(FUSED_56, _sched(th=2, uy=28, total_units=2240 + 77, half_from=2240 - 76, lazy_queue=1), "half_from")


def test_rejects_nh_beyond_the_clamp():
    # 2 static rounds + one more of 160 teams = 480 units handed out before the halves may start: nh <= 640
    ok = _sched(th=4, uy=14, total_units=1120 + 640, half_from=480, lazy_queue=1, teams=160)
    hipref.check_sched(FUSED_56, ok)
    _rejected(FUSED_56, dict(ok, total_units=1120 + 641, half_from=479), "half_from")


def test_rejects_a_dict_without_every_field():
    s = _sched(total_units=1792, th=4, tw=112)
    del s["roles"]
    with pytest.raises(AssertionError):
        hipref.check_sched(ROLES_112, s)
