"""Tile geometry and case lists of the H = 512 attention instances (tests/test_attention512_cpu.py, tests/test_attention512_gpu.py).

attention_ref.rows_per_pass(512) is 0 -- its formula has H / 4 lanes per row, and a row of 512 features takes the whole wave with NV = 2 pieces per
lane -- so the width has its own helper: min(H / 4, 64) lanes per row, one row per wave, R = 8 rows per pass, R * AU = 32 rows per loop trip.
Reference, inputs, flatness and the ceiling are attention_ref's.
"""
import attention_ref as A

H = 512
LANES = min(H // 4, 64)                              # lanes per row
NV = (H // 4) // LANES                               # 16-byte pieces per lane and half-row
R = (A.AT // 64) * (64 // LANES)                     # rows per pass


def cached(T):
    """(forward cached, backward cached): the launcher's arithmetic, fixed + max(T, R) H 4 <= LDS_MAX."""
    Tp = (T + 3) & ~3
    body = max(T, R) * H * 4
    return (Tp + 32) * 4 + body <= A.LDS_MAX, (2 * Tp + 32) * 4 + body <= A.LDS_MAX


# 1; R - 1, R, R + 1; R AU - 1, R AU, R AU + 1; 2 R AU + 3; the last cached T and the first re-read one; a second trip of the t += AT softmax loops
T_LIST = (1, 7, 8, 9, 31, 32, 33, 67, 79, 80, 513)
ZEROS_T = (33, 80)                                   # one cached, one re-reading
UNIT_T = 33                                          # the unit and saturated cases (chosen by attention_ref.dpre_condition, see the CPU test)
EXACT_T = (33, 80)


def dense_B(T):
    """1 - 3 utterances."""
    return 1 + (H // 64 + T) % 3


def flat_family():
    """Every (T, B, ragged, scale) the GPU file runs against the derived bounds."""
    seen = []
    for T in T_LIST:
        seen.append((T, dense_B(T), False, 'flat')); seen.append((T, A.RAGGED_B, True, 'flat'))
    for T in ZEROS_T:
        seen.append((T, dense_B(T), False, 'zeros')); seen.append((T, A.RAGGED_B, True, 'zeros'))
    return seen
