"""CPU restatement (numpy fp32) of the two ends of an `mcts` decision of the agent loop -- the authority for csrc/agent_mcts.hip.  Test
infrastructure only.

  root(Qpi, u, ...)        : mcts.py:166-170 of the reference with the draw of efe_agent_choose's `probs` mode (agent_ref.draw over A actions):
                             thr = max(Qpi) - (sum left to right) / A in float32; -> choice, decided, active and the queue written
  walk(N, child, e)        : Node.action_selection's walk on the planner's arrays (BatchedMCTS._most_visited_paths for one slot, with the
                             root-only tree spelled out instead of left to numpy's negative index)
  enqueue(...)             : _most_visited_paths + _trim_path + test_demo.py:167-170 on numpy copies of the efe_agent arrays
  random_tree / chain_tree : synthetic [cap][A] trees"""
import numpy as np

F = np.float32


def draw(p, u):
    """agent_ref.draw for len(p) actions: cdf = cumsum(p) / cumsum(p)[-1] in float32, the first edge above u; u == 1.0: the last p > 0"""
    p = np.asarray(p, dtype=F)
    if not np.all(np.isfinite(p)) or np.any(p < 0):
        return -1
    cdf = np.zeros(len(p), dtype=F)
    acc = F(0)
    for k in range(len(p)):
        acc = p[k] if k == 0 else F(acc + p[k])
        cdf[k] = acc
    with np.errstate(all='ignore'):
        cdf = (cdf / cdf[-1]).astype(F)
    for k in range(len(p)):
        if cdf[k] > F(u):
            return k
    pos = np.flatnonzero(p > 0)
    return int(pos[-1]) if len(pos) else -1


def threshold_value(q):
    """max - mean with the mean as the left-to-right float32 sum over A"""
    q = np.asarray(q, dtype=F)
    acc = q[0]
    for k in range(1, len(q)):
        acc = F(acc + q[k])
    return F(q.max() - F(acc / F(len(q))))


def root(Qpi, u, use_habit, threshold, jumps):
    """-> choice [n] int32, decided [n] uint8, active [n] uint8, queues (list of lists; None = the queue is not touched)"""
    Qpi = np.asarray(Qpi, dtype=F)
    n = Qpi.shape[0]
    choice, decided, active, queues = np.zeros(n, np.int32), np.zeros(n, np.uint8), np.zeros(n, np.uint8), []
    for i in range(n):
        q = Qpi[i]
        if not np.all(np.isfinite(q)) or np.any(q < 0):
            choice[i], decided[i], active[i] = -1, 1, 0
            queues.append([])
        elif use_habit and threshold_value(q) > F(threshold):
            c = draw(q, u[i])
            choice[i], decided[i], active[i] = c, 1, 0
            queues.append([] if c < 0 else [c] * jumps)
        else:
            choice[i], decided[i], active[i] = -2, 0, 1
            queues.append(None)
    return choice, decided, active, queues


def walk(N, child, e):
    """visited actions of slot e: argmax of N (first index on ties) down to the first node whose child[.][0] < 0"""
    visited, node = [], 0
    while True:
        a = int(np.argmax(N[e, node]))
        visited.append(a)
        node = int(child[e, node, a])
        if node < 0 or child[e, node, 0] < 0:
            return visited


def enqueue(N, child, ids, decided, queue, head, length, jumps):
    """the arrays of efe_agent after efe_agent_mcts_enqueue (copies) and the trimmed paths (None for decided slots)"""
    from daimc_amd.mcts import BatchedMCTS, _trim_path
    A = N.shape[2]
    queue, head, length = queue.copy(), head.copy(), length.copy()
    visited = BatchedMCTS._most_visited_paths(N, child)
    paths = []
    for i, g in enumerate(ids):
        if decided[i]:
            paths.append(None)
            continue
        assert visited[i] == walk(N, child, i), i
        path = _trim_path(visited[i], A)
        paths.append(path)
        q = [a for a in path for _ in range(jumps)]
        queue[g, :len(q)] = q
        head[g], length[g] = 0, len(q)
    return queue, head, length, paths


def chain_tree(actions, cap, A, rng=None):
    """N / child [cap][A] of a tree whose most-visited path is `actions` (every node on it expanded, the last child not)"""
    N = np.zeros((cap, A), F)
    child = np.full((cap, A), -1, np.int32)
    node, nxt = 0, 1
    for a in actions:
        N[node] = 1.0 if rng is None else rng.integers(1, 4, size=A).astype(F)
        N[node, a] = N[node].max() + 1.0
        child[node] = np.arange(nxt, nxt + A)
        node, nxt = nxt + a, nxt + A
    assert nxt <= cap - 1                                             # (the last node stays unexpanded)
    return N, child


def random_tree(rng, cap, A, expansions, ties=False):
    """a tree grown like the planner's: the root is expanded, then `expansions` times a random unexpanded node; random visit counts"""
    N = np.zeros((cap, A), F)
    child = np.full((cap, A), -1, np.int32)
    leaves, nxt = [0], 1
    for _ in range(1 + expansions):
        node = leaves.pop(int(rng.integers(len(leaves))))
        child[node] = np.arange(nxt, nxt + A)
        N[node] = rng.integers(1, 3 if ties else 50, size=A).astype(F)
        leaves += list(range(nxt, nxt + A))
        nxt += A
    assert nxt <= cap - 1
    return N, child
