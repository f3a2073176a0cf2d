"""The shape-edge cases of the three learner families (test infrastructure): one table for tests/test_policy_shapes_cpu.py,
tests/test_gpu_policy_shapes.py, tests/test_gpu_sac_shapes.py and tests/test_gpu_td3_shapes.py.

The host plans accept obs_dim 1..4096, act_dim 1..16, one to three hidden layers of widths 16..256 in steps of 16.  The older files
run (D, A) in {(10, 7), (25, 4), (25, 8), (25, 7)}, one or two layers, widths from {16, 32, 48, 64} or 256 x 256.  The cases below are
the smallest shapes that reach what those leave out.  The trunks are entries of ``TRUNKS`` in tests/indep_policy.py, indep_sac.py,
indep_sac_update.py and indep_td3.py (pi, then vf for ActorCritic and qf for the others):

    32x48x16-tanh-16x48x32     three layers (n == 3: sel4(x, 2), nt[2], last_tiles, R.x[3]), MT = 4, all widths different: a select
                               that picks another layer's width or weights changes the result
    80x16x112-relu-96x240x16   three layers, MT = 16 with partial tiles (5, 1, 7 and 6, 15, 1 tiles of 16), a wide layer next to a
                               16-wide one; the dW block lists at capacity (9 entries for PPO, 10 for the critics) with ragged tiles
    32-relu-80                 a narrow actor (MT = 4, 16 parts) and a wide critic (MT = 16, 4 parts) in one update
    144x16-tanh-48             a wide actor and a narrow critic
    64x64x64-relu              the block lists at capacity with full tiles

The cases (D, A, trunk, B).  Features = D + 6; kb0 = ceil(features / 4) first-layer k-blocks; fr = features padded to 16 rows:

    (12, 13, 80x16x112-relu-96x240x16, 75)   18 features, kb0 = 5 (kb0 % 4 != 0: `kb < nkb` is false for three k-blocks of the second
                                             column block), fr = 32, two padding columns; A = 13: noise pairs 4..6, the second value
                                             of the last pair dropped, the log-prob over four lanes, action k-blocks 2 and 3, three
                                             action columns zeroed in dW
    (45, 16, 32-relu-80, 75)                 51 features, kb0 = 13, fr = 64; a full head: pairs 0..7, no action padding
    (12, 9, 144x16-tanh-48, 75)              A = 9: lane g = 2 carries one component, pair 4's second value dropped
    (45, 13, 64x64x64-relu, 75)              capacity block lists at kb0 = 13 and A = 13
    (12, 9, 32x48x16-tanh-16x48x32, 75)      three layers of different widths at kb0 = 5
    (1, 1, 32x48x16-tanh-16x48x32, 33)       7 features, kb0 = 2; A = 1: the second value dropped in the first pair; two full tiles
                                             and a tile of one row
    (58, 1, 80x16x112-relu-96x240x16, 33)    64 features exactly: kb0 = 16, fr = 64, no padding column
    (1, 16, 32-relu-80, 1)                   one row, a full head on the smallest observation
    (45, 16, 32-relu-80, 600)                38 tiles: 13 parts of 3 for the actor, 4 parts of 10 for the critic in one update

The A = 1 cases have B = 33: one action component cannot meet TD3's clamp census in 75 rows (it gave 3 rows at (1, 1)), and 33 is
below the census' threshold of 75, as B = 1 is.  For the same reason SAC's "both clamp bounds of log_std act somewhere" is asserted
only where the float64 reference's own log_std shows both, which is every case with A >= 9.  The forward-only tests use N = 40
environments for the collection call and the table's B rows for the batch entries."""
import torch

N = 40
CASES = [(12, 13, "80x16x112-relu-96x240x16", 75), (45, 16, "32-relu-80", 75), (12, 9, "144x16-tanh-48", 75), (45, 13, "64x64x64-relu", 75),
         (12, 9, "32x48x16-tanh-16x48x32", 75), (1, 1, "32x48x16-tanh-16x48x32", 33), (58, 1, "80x16x112-relu-96x240x16", 33),
         (1, 16, "32-relu-80", 1), (45, 16, "32-relu-80", 600)]
TRUNK_NAMES = ("32x48x16-tanh-16x48x32", "80x16x112-relu-96x240x16", "32-relu-80", "144x16-tanh-48", "64x64x64-relu")
THREE_LAYER_75 = [(12, 13, "80x16x112-relu-96x240x16", 75), (12, 9, "32x48x16-tanh-16x48x32", 75)]      # also: the steps in SB3's order
BIT_CASES = THREE_LAYER_75 + [(45, 16, "32-relu-80", 600)]                                                # equal inputs, equal bits
STRAY_CASES = [(45, 16, "32-relu-80", 75), (1, 1, "32x48x16-tanh-16x48x32", 33), (58, 1, "80x16x112-relu-96x240x16", 33)]
ROW_CASES = [(45, 16, "32-relu-80", 75), (12, 13, "80x16x112-relu-96x240x16", 75)]                          # A = 16 and A = 13
TD3_CASES = [c + (2,) for c in CASES] + [c + (1,) for c in THREE_LAYER_75]
CPU_DIMS = ((1, 1), (12, 9), (12, 13), (45, 16), (58, 1))
SENTINEL, BORDER = 1234.5, 64


def tiles(B: int) -> int:
    return (B + 15) // 16


def parts(B: int, widest: int) -> int:
    """The split of a batch's tiles into parts, restated: at most 16 parts up to width 64, at most 4 above."""
    most = 16 if widest <= 64 else 4
    per = (tiles(B) + most - 1) // most
    return (tiles(B) + per - 1) // per


def padding_columns(pack, zeros: dict, key: str, cols: slice, padded: int) -> torch.Tensor:
    """The blob positions of one weight matrix' padding columns, found through ``pack`` alone: a state dict of zeros with ones in
    ``zeros[key][:, cols]`` marks the real positions; its block of the blob starts at the first of them (row 0, column 0 of the
    block comes first in both tile orders) and holds rows x ``padded`` floats; the others are the padding."""
    sd = {k: v.clone() for k, v in zeros.items()}
    sd[key][:, cols] = 1.0
    real = pack(sd) != 0
    rows, n = sd[key].shape[0], int(sd[key][0].sum())
    start = int(real.nonzero()[0])
    mask = torch.zeros_like(real)
    mask[start:start + rows * padded] = True
    assert int((mask & real).sum()) == int(real.sum()) == rows * n
    mask &= ~real
    assert int(mask.sum()) == rows * (padded - n)
    return mask


def bordered(n: int, fill=None):
    """-> (a tensor of n + 2 BORDER floats holding SENTINEL, its middle slice of n floats, holding ``fill`` where given)."""
    full = torch.full((n + 2 * BORDER,), SENTINEL, device="cuda")
    if fill is not None:
        full[BORDER:BORDER + n] = fill
    return full, full[BORDER:BORDER + n]


def borders_intact(full: torch.Tensor) -> bool:
    return bool((full[:BORDER] == SENTINEL).all()) and bool((full[-BORDER:] == SENTINEL).all())
