"""CPU tier: where the fused solve + sweep launch runs its role-split form (kccot_sinkhorn_fused_roles_eligible).  Two roles of
ceil64(n x lanes per line) threads must fit one 1024-thread workgroup: n <= 32 at 16 lanes per line, n <= 64 at 8 or 4;
everything else, and option "sinkhorn_fused_roles" = 0, keeps the one-role kernel.  No launch is made."""
import pytest


@pytest.fixture()
def L():
    from kccotgan_amd import _lib
    defaults = {k: _lib.get_option(k) for k in _lib.option_names()}
    yield _lib
    for k, v in defaults.items():
        _lib.set_option(k, v)


# (n, sinkhorn_lanes_per_line, sinkhorn_fused_max_n) -> the role kernel runs.  lanes = 0 is the default rule: 16 lanes per
# line up to n = 32, 8 above; the lanes option only applies to 32 < n <= 64.
TABLE = [
    (1, 0, 64, True), (16, 0, 64, True), (17, 0, 64, True), (32, 0, 64, True),      # 16 lanes: 2 x ceil64(16 n) <= 1024
    (32, 4, 64, True), (32, 8, 64, True),                                           # the option does not reach n <= 32
    (33, 0, 64, True), (40, 0, 64, True), (64, 0, 64, True), (64, 8, 64, True),     # 8 lanes: 2 x ceil64(8 n) <= 1024
    (33, 4, 64, True), (64, 4, 64, True),                                           # 4 lanes
    (33, 16, 64, False), (48, 16, 64, False), (64, 16, 64, False),                  # 16 lanes above 32: 2 x 576 .. 2 x 1024
    (65, 0, 128, False), (100, 0, 128, False), (128, 0, 128, False),                # <16, 8>: 2 x 576 .. 2 x 1024
    (100, 4, 128, False),
]


@pytest.mark.parametrize("n,lanes,max_n,want", TABLE)
def test_role_kernel_is_taken_where_both_roles_fit_one_workgroup(L, n, lanes, max_n, want):
    with L.options(sinkhorn_fused_roles=1, sinkhorn_lanes_per_line=lanes, sinkhorn_fused_max_n=max_n):
        assert L.lib.kccot_sinkhorn_fused_eligible(n, 100) == 1
        assert L.lib.kccot_sinkhorn_fused_roles_eligible(n, 100) == int(want)
        with L.options(sinkhorn_fused_roles=0):
            assert L.lib.kccot_sinkhorn_fused_roles_eligible(n, 100) == 0


def test_role_kernel_needs_the_fused_launch_itself(L):
    with L.options(sinkhorn_fused_roles=1):
        assert L.lib.kccot_sinkhorn_fused_roles_eligible(64, 100) == 1
        assert L.lib.kccot_sinkhorn_fused_roles_eligible(64, 288) == 0          # the dual history no longer fits the LDS
        assert L.lib.kccot_sinkhorn_fused_roles_eligible(65, 100) == 0          # sinkhorn_fused_max_n = 64
        assert L.lib.kccot_sinkhorn_fused_roles_eligible(0, 100) == 0
        with L.options(sinkhorn_fused=0):
            assert L.lib.kccot_sinkhorn_fused_roles_eligible(64, 100) == 0
