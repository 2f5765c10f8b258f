"""What the wrappers of the two RANSAC terms (eight_point.py, pnp.py) share: the workspace layout of csrc/dfe_ransac.h and the
checks of the arguments both entry points take."""
import torch

MAX_NUM = 16384
MAX_HYP = 4096


def workspace_sections(B, num, hyp, match_doubles, hyp_doubles, first_name, hyp_name):
    """Byte offsets of the five sections of a RANSAC workspace (each starts on 16 bytes): the matches [2B,num,match_doubles] and
    the hypotheses [2B,hyp,hyp_doubles] in double under the names given, then int32 ``counts`` [2B,hyp], ``w1`` and ``w2``
    [2B,num]; ``bytes`` is the total."""
    r16 = lambda v: (v + 15) // 16 * 16   # noqa: E731
    hyps = 16 * match_doubles * B * num
    counts = hyps + r16(16 * hyp_doubles * B * hyp)
    w1 = counts + r16(8 * B * hyp)
    w2 = w1 + r16(8 * B * num)
    return {first_name: 0, hyp_name: hyps, "counts": counts, "w1": w1, "w2": w2, "bytes": w2 + r16(8 * B * num)}


def check_draw(flow_bwd0, flow_fwd0, idx, pick, sets, set_size, name, solver):
    """The shapes and dtypes of (two fp32 flows [B,2,H,W], idx int32 [2B,k], pick int64 [num], sets int32 [B,hyp,set_size]) and
    the limits of the draw -> (B, H, W, k, num, hyp).  ``name`` prefixes the ValueErrors; ``solver`` is who needs set_size matches."""
    if flow_bwd0.dim() != 4 or flow_bwd0.shape[1] != 2 or flow_fwd0.shape != flow_bwd0.shape:
        raise ValueError("%s: two flows [B,2,H,W] of one scale expected" % name)
    B, _, H, W = flow_bwd0.shape
    if idx.dtype != torch.int32 or idx.dim() != 2 or idx.shape[0] != 2 * B or pick.dtype != torch.int64 or pick.dim() != 1:
        raise ValueError("%s: idx int32 [2B,k] and pick int64 [num] expected" % name)
    if sets.dtype != torch.int32 or sets.dim() != 3 or sets.shape[0] != B or sets.shape[2] != set_size:
        raise ValueError("%s: sets int32 [B,hyp,%d] expected" % (name, set_size))
    k, num, hyp = idx.shape[1], pick.shape[0], sets.shape[1]
    if num < set_size:
        raise ValueError("%s needs at least %d matches (got %d)" % (solver, set_size, num))
    if num > MAX_NUM or hyp > MAX_HYP or hyp < 1:
        raise ValueError("%s: at most %d matches and 1 to %d hypotheses (got %d, %d)" % (name, MAX_NUM, MAX_HYP, num, hyp))
    if k > H * W or k < 1:
        raise ValueError("%s: 1 <= k <= H*W expected" % name)
    return B, H, W, k, num, hyp
