"""numpy restatements of the rules behind the record of an agent run (csrc/agent_trace.hip), written from the rules as DESIGN states them:
the plan mask (the demo's make_mask), the filmed frame (marker, mask, saturating uint8) and the edge rule of the action draw that
efe_agent_choose documents.  fp32 throughout; the tests compare bit for bit."""
import numpy as np

F32 = np.float32


def start(v):
    """int(v) clamped to 0..31; a NaN starts at 0"""
    v = F32(v)
    if not v >= 0:
        return 0
    return int(v) if v <= 31 else 31


def plan_mask(paths, state, jumps):
    """paths: the explored action lists of one decision; state: the game's 7 floats -> [32, 32] float32"""
    count = np.zeros((32, 32), dtype=np.int32)
    for path in paths:
        tx, ty = start(state[5]), start(state[4])
        for a in path:
            for _ in range(jumps):
                if a == 0 and tx < 31:
                    tx += 1
                elif a == 1 and tx > 0:
                    tx -= 1
                elif a == 2 and ty < 31:
                    ty += 1
                elif a == 3 and ty > 0:
                    ty -= 1
                else:
                    continue                                         # a blocked move adds nothing
                count[tx, ty] += 1
    top = count.max()
    if top == 0:
        return np.zeros((32, 32), dtype=F32)                         # a decision that explored nothing
    return count.astype(F32) / F32(top)


def history_paths(H_act, H_len, H_active, n_iter, slot):
    """the explored paths of `slot`: the history rows below n_iter in which the episode was live, cut to their length"""
    return [list(H_act[r, slot, :H_len[r, slot]]) for r in range(n_iter) if H_active[r, slot]]


def view(frame, mask=None):
    """frame [64, 64] float32 -> [64, 64] uint8: marker, mask over rows and columns 16..47, uint8(min(trunc(v * 255), 255)), NaN -> 0"""
    v = np.array(frame, dtype=F32).reshape(64, 64).copy()
    v[59:63, 31] = F32(1.0)
    if mask is not None:
        v[16:48, 16:48] = v[16:48, 16:48] + np.asarray(mask, dtype=F32).reshape(32, 32)
    with np.errstate(invalid='ignore'):
        s = np.minimum(np.trunc(v * F32(255.0)), F32(255.0))
    s = np.where(np.isnan(v), F32(0.0), s)
    return s.astype(np.uint8)


def choice(p, u):
    """np.random.choice(4, p = p) at the uniform u, as efe_agent_choose documents it: -1 for a p with a NaN, an infinite or a negative
    entry; cdf = cumsum(p) / cumsum(p)[3] (fp32, left to right), the first edge above u; at u == 1.0 the last action with p > 0"""
    p = np.asarray(p, dtype=F32)
    if not np.all((p >= 0) & (p <= np.finfo(F32).max)):
        return -1
    cdf = np.zeros(4, dtype=F32)
    cdf[0] = p[0]
    for k in range(1, 4):
        cdf[k] = cdf[k - 1] + p[k]
    with np.errstate(invalid='ignore', divide='ignore'):
        edges = cdf / cdf[3]
    for k in range(4):
        if edges[k] > F32(u):
            return k
    c = -1
    for k in range(4):
        if p[k] > 0:
            c = k
    return c
