#!/usr/bin/env python
"""The repack of ModelDown's optimiser step at every admitted geometry (csrc/train_down_g.hip k_repack_down_g), restated in numpy.

Two independent restatements per packed form of the generic path:
  pack_*   the HOST packer of engine_weights.hip (pack_heads / pack_encoder / pack_decoder under ctx->generic): loops over the destination
           in the packer's own order, reading the tensor in torch's shape
  Table    the table build_down_repack_g builds (offsets into the flat master copy from EncGeo / DecHeadGeo / DecTailGeo) and, per entry,
           the kernel's destination -> source map: owner thread i of an entry -> the destination floats it writes and, for each, the index
           in the master copy it reads (-1: a written zero)

check(C, R) packs a master copy whose element j holds the value j + 1 (so a gathered value names its source), runs both, and asserts that
  * every destination float of every packed buffer has exactly ONE owning thread (the 128-byte-segment thread order included),
  * the value the map gathers is the value the host packer put there, element for element, and padding is a written zero.
python tools/emulate_repack_g.py         all 75 geometries (1..3 channels x resolutions 32..128 in steps of 4)"""
import sys

import numpy as np

RES = list(range(32, 129, 4))
DT_W = (0, 36928, 73856)                 # po_net.13 / .15 / .17 weights in the tail (kernels.h DT_W1..3); biases behind each
DT_B = (36864, 73792, 92288)
DT_W4 = 92320
DH = ((0, 2560, 256, 10), (2816, 68352, 256, 256), (68608, 134144, 256, 256))      # kernels.h DH_W0.., (w, b, out, in)
DH_W3 = 134400
EQS = ((0, 65536, 256, 256), (65792, 131328, 256, 256), (131584, 136704, 20, 256))   # kernels.h EQS_*, inside the ENC_SMALL_P part
ENC_SMALL_P = 136724
CT = ((64, 64), (64, 64), (32, 64))      # (out, in) of po_net.13 / .15 / .17


def extents(R):
    hs = []
    for _ in range(4):
        R = (R - 3) // 2 + 1
        hs.append(R)
    return hs


class Geo:
    """EncGeo, DecHeadGeo and DecTailGeo of kernels.h"""

    def __init__(self, C, R):
        self.C, self.R = C, R
        self.B = 16 if R == 32 else R // 4
        self.H4 = extents(R)[3]
        self.K = 64 * self.H4 ** 2
        self.F = 64 * self.B ** 2
        enc_conv = ((32, C), (32, 32), (64, 32), (64, 64))
        off, self.ew, self.eb = 0, [], []
        for out, cin in enc_conv:
            self.ew.append(off); off += out * cin * 9
            self.eb.append(off); off += out
        self.enc_conv = enc_conv
        self.w9, self.b9 = off, off + 256 * self.K
        self.small = self.b9 + 256
        self.D = self.small + ENC_SMALL_P                       # EncGeo::P(): where po_net begins
        self.b3 = DH_W3 + self.F * 256
        self.T = self.D + self.b3 + self.F                      # where the ConvT tail begins
        self.P = self.T + DT_W4 + 289 * C


# ---- the host packers ------------------------------------------------------------------------------------------------
def upload_packed(ntaps, cout, cin, get):
    """[tap][mtile][kc][lane][4] of v_mfma_f32_32x32x2_f32"""
    mtiles, KC = (cout + 31) // 32, (cin + 7) // 8
    p = np.zeros((ntaps, mtiles, KC, 64, 4))
    for t in range(ntaps):
        for mt in range(mtiles):
            for kc in range(KC):
                for lane in range(64):
                    co = mt * 32 + (lane & 31)
                    for s in range(4):
                        ci = kc * 8 + 4 * (lane >> 5) + s
                        if co < cout and ci < cin:
                            p[t, mt, kc, lane, s] = get(t, co, ci)
    return p.reshape(-1)


def upload_packed_fast(ntaps, cout, cin, W3):
    """the same from an array W3[tap][co][ci] (vectorised: the large Linears)"""
    mtiles, KC = (cout + 31) // 32, (cin + 7) // 8
    pad = np.zeros((ntaps, mtiles * 32, KC * 8))
    pad[:, :cout, :cin] = W3
    p = pad.reshape(ntaps, mtiles, 32, KC, 2, 4).transpose(0, 1, 3, 4, 2, 5)       # [t][mt][kc][lane >> 5][lane & 31][s]
    return p.reshape(-1)


def nhwc_perm(channels, positions):
    p, c = np.meshgrid(np.arange(positions), np.arange(channels), indexing='ij')
    return (c * positions + p).reshape(-1)


def pad_bias(b, n):
    out = np.zeros(n)
    out[:len(b)] = b
    return out


def pack_linear(W, b, row_perm=None, col_perm=None):
    out, cin = (len(row_perm) if row_perm is not None else W.shape[0]), W.shape[1]
    Wp = W[row_perm] if row_perm is not None else W
    Wp = Wp[:, col_perm] if col_perm is not None else Wp
    bp = b[row_perm] if row_perm is not None else b
    return upload_packed_fast(1, out, cin, Wp[None]), pad_bias(bp, (out + 31) // 32 * 32)


def pack_linear16(W, b, col_perm=None):
    out, cin = W.shape
    mtiles, KC = (out + 15) // 16, (cin + 15) // 16
    Wp = W[:, col_perm] if col_perm is not None else W
    pad = np.zeros((mtiles * 16, KC * 16))
    pad[:out, :cin] = Wp
    p = pad.reshape(mtiles, 16, KC, 4, 4).transpose(0, 2, 3, 1, 4)                 # [mt][kc][lane >> 4][lane & 15][s]
    return p.reshape(-1), pad_bias(b, mtiles * 16)


def pack_conv(W, b, transposed):
    """W [cout][cin][3][3] (Conv2d) or [cin][cout][3][3] (ConvTranspose2d) as nine taps"""
    if transposed:
        cin, cout = W.shape[:2]
        get = lambda t, co, ci: W[ci, co].reshape(9)[t]
    else:
        cout, cin = W.shape[:2]
        get = lambda t, co, ci: W[co, ci].reshape(9)[t]
    return upload_packed(9, cout, cin, get), pad_bias(b, (cout + 31) // 32 * 32)


def pack_enc1p(W, C):
    p = np.zeros((9, 64, 2))
    for t in range(9):
        for lane in range(64):
            for i in range(2):
                co, ci = lane & 31, 2 * i + (lane >> 5)
                if ci < C:
                    p[t, lane, i] = W[co, ci].reshape(9)[t]
    return p.reshape(-1)


def pack_wf(W, C):
    p = np.zeros((9, 32, 4))
    for t in range(9):
        for ci in range(32):
            for c in range(C):
                p[t, ci, c] = W[ci, c].reshape(9)[t]
    return p.reshape(-1)


def host_pack(g, flat):
    """every packed buffer of the generic path from the flat master copy -> {name: array}"""
    C, B, K, F = g.C, g.B, g.K, g.F
    t = lambda off, *shape: flat[off:off + int(np.prod(shape))].reshape(shape)
    out = {}
    for i, (w, b, o, n) in enumerate(DH):
        W, bb = t(g.D + w, o, n), t(g.D + b, o)
        out[f'dec_fc{i}.w'], out[f'dec_fc{i}.b'] = pack_linear(W, bb)
        out[f'dec16_{i}.w'], out[f'dec16_{i}.b'] = pack_linear16(W, bb)
    for i, (w, b, o, n) in enumerate(EQS):
        W, bb = t(g.small + w, o, n), t(g.small + b, o)
        out[f'enc_fc{i + 1}.w'], out[f'enc_fc{i + 1}.b'] = pack_linear(W, bb)
        out[f'enc16_{i + 1}.w'], out[f'enc16_{i + 1}.b'] = pack_linear16(W, bb)
    for i, (o, n) in enumerate(g.enc_conv):
        out[f'g_enc{i}.w'], out[f'g_enc{i}.b'] = pack_conv(t(g.ew[i], o, n, 3, 3), t(g.eb[i], o), False)
    out['g_enc1p'] = pack_enc1p(t(g.ew[0], 32, C, 3, 3), C)
    colp = nhwc_perm(64, g.H4 ** 2)
    W9, b9 = t(g.w9, 256, K), t(g.b9, 256)
    out['enc_fc0.w'], out['enc_fc0.b'] = pack_linear(W9, b9, col_perm=colp)
    out['enc16_0.w'], out['enc16_0.b'] = pack_linear16(W9, b9, col_perm=colp)
    out['g_fc4.w'], out['g_fc4.b'] = pack_linear(t(g.D + DH_W3, F, 256), t(g.D + g.b3, F), row_perm=nhwc_perm(64, B * B))
    for i, (o, n) in enumerate(CT):
        out[f'g_ct{i}.w'], out[f'g_ct{i}.b'] = pack_conv(t(g.T + DT_W[i], n, o, 3, 3), t(g.T + DT_B[i], o), True)
    out['g_wf'] = pack_wf(t(g.T + DT_W4, 32, C, 3, 3), C)
    return out


# ---- the kernel's maps -----------------------------------------------------------------------------------------------
BIAS, DENSE32, DENSE16, CONV32, CONVT32, ENC1P, WF4 = range(7)


def perm_of(i, channels, positions):
    return (i % channels) * positions + i // channels if channels else i


class Table:
    """build_down_repack_g: entries (name, src, kind, n, out, in, KC, mtiles, row, col, vec, swizzle), block0 ascending"""

    def __init__(self, g):
        self.e, self.blocks = [], 0
        C, B = g.C, g.B
        for i, (w, b, o, n) in enumerate(DH):
            self.dense32(f'dec_fc{i}', g.D + w, g.D + b, o, n); self.dense16(f'dec16_{i}', g.D + w, g.D + b, o, n)
            ew, eb, eo, en = EQS[i]
            self.dense32(f'enc_fc{i + 1}', g.small + ew, g.small + eb, eo, en); self.dense16(f'enc16_{i + 1}', g.small + ew, g.small + eb, eo, en)
        for i, (o, n) in enumerate(g.enc_conv):
            self.conv32(f'g_enc{i}', CONV32, g.ew[i], g.eb[i], o, n)
        self.add('g_enc1p', g.ew[0], ENC1P, 1152, 32, C, 0, 0)
        self.dense32('enc_fc0', g.w9, g.b9, 256, g.K, col=(64, g.H4 ** 2)); self.dense16('enc16_0', g.w9, g.b9, 256, g.K, col=(64, g.H4 ** 2))
        self.dense32('g_fc4', g.D + DH_W3, g.D + g.b3, g.F, 256, row=(64, B * B))
        for i, (o, n) in enumerate(CT):
            self.conv32(f'g_ct{i}', CONVT32, g.T + DT_W[i], g.T + DT_B[i], o, n)
        self.add('g_wf', g.T + DT_W4, WF4, 1152, C, 32, 0, 0)

    def add(self, name, src, kind, n, out, cin, KC, mtiles, row=(0, 0), col=(0, 0)):
        vec = kind in (DENSE32, DENSE16) and not col[0] and src % 4 == 0 and cin % (8 if kind == DENSE32 else 16) == 0
        swz = kind == DENSE32 and vec and KC % 4 == 0
        self.e.append(dict(name=name, src=src, kind=kind, n=n, block0=self.blocks, out=out, cin=cin, KC=KC, mtiles=mtiles, row=row, col=col, vec=vec, swizzle=swz))
        self.blocks += (n + 255) // 256

    def bias(self, name, src, out, n, row=(0, 0)):
        self.add(name, src, BIAS, n, out, 0, 0, 0, row)

    def dense32(self, name, w, b, out, cin, row=(0, 0), col=(0, 0)):
        mtiles, KC = (out + 31) // 32, (cin + 7) // 8
        self.add(name + '.w', w, DENSE32, mtiles * KC * 64, out, cin, KC, mtiles, row, col)
        self.bias(name + '.b', b, out, mtiles * 32, row)

    def dense16(self, name, w, b, out, cin, col=(0, 0)):
        mtiles, KC = (out + 15) // 16, (cin + 15) // 16
        self.add(name + '.w', w, DENSE16, mtiles * KC * 64, out, cin, KC, mtiles, (0, 0), col)
        self.bias(name + '.b', b, out, mtiles * 16)

    def conv32(self, name, kind, w, b, out, cin):
        mtiles, KC = (out + 31) // 32, (cin + 7) // 8
        self.add(name + '.w', w, kind, 9 * mtiles * KC * 64, out, cin, KC, mtiles)
        self.bias(name + '.b', b, out, mtiles * 32)


def entry_map(d):
    """-> (dst [n x width] destination float index per owner and slot, src the same shape: index in the master copy or -1 = zero)"""
    i = np.arange(d['n'])
    k = d['kind']
    if k == BIAS:
        ch, pos = d['row']
        s = np.where(i < d['out'], d['src'] + ((i % ch) * pos + i // ch if ch else i), -1)
        return i[:, None], s[:, None]
    if k == ENC1P:
        kk, lane, t = i & 1, (i >> 1) & 63, i >> 7
        co, ci = lane & 31, 2 * kk + (lane >> 5)
        return i[:, None], np.where(ci < d['cin'], d['src'] + (co * d['cin'] + ci) * 9 + t, -1)[:, None]
    if k == WF4:
        c, ci, t = i & 3, (i >> 2) & 31, i >> 7
        return i[:, None], np.where(c < d['out'], d['src'] + (ci * d['out'] + c) * 9 + t, -1)[:, None]
    if d['swizzle']:
        t = i & 255
        l, c4 = t >> 3, t & 7
        i = (i & ~255) | ((c4 >> 1) * 64 + (c4 & 1) * 32 + l)
    lane, r = i & 63, i >> 6
    s4 = np.arange(4)[None, :]
    if k in (DENSE32, DENSE16):
        w, q = (32, 5) if k == DENSE32 else (16, 4)
        kc, mt = r % d['KC'], r // d['KC']
        co = mt * w + (lane & (w - 1))
        ci = ((kc * 8 + 4 * (lane >> 5)) if k == DENSE32 else (kc * 16 + 4 * (lane >> 4)))[:, None] + s4
        rch, rpos = d['row'] if k == DENSE32 else (0, 0)
        row = (co % rch) * rpos + co // rch if rch else co
        cch, cpos = d['col']
        col = (ci % cch) * cpos + ci // cch if cch else ci
        ok = (co < d['out'])[:, None] & (ci < d['cin'])
        src = np.where(ok, d['src'] + row[:, None] * d['cin'] + col, -1)
        if d['vec']:        # one aligned float4 of the row: the four indices are consecutive and the first a multiple of 4
            live = src[:, 0] >= 0
            assert np.all(src[live, 0] % 4 == 0) and np.all(np.diff(src[live], axis=1) == 1), d['name']
    else:
        kc = r % d['KC']; r2 = r // d['KC']
        mt, tap = r2 % d['mtiles'], r2 // d['mtiles']
        co = (mt * 32 + (lane & 31))[:, None]
        ci = (kc * 8 + 4 * (lane >> 5))[:, None] + s4
        ok = (co < d['out']) & (ci < d['cin'])
        idx = (co * d['cin'] + ci) * 9 if k == CONV32 else (ci * d['out'] + co) * 9
        src = np.where(ok, d['src'] + idx + tap[:, None], -1)
    return i[:, None] * 4 + s4, src


def find_entry(table, block):
    """the kernel's binary search over block0"""
    e, hi = 0, len(table.e) - 1
    while e < hi:
        mid = (e + hi + 1) >> 1
        if block >= table.e[mid]['block0']:
            e = mid
        else:
            hi = mid - 1
    return e


def check(C, R):
    g = Geo(C, R)
    flat = np.arange(1, g.P + 1, dtype=np.float64)           # element j holds j + 1: exact in fp64, and 0 is "padding"
    want = host_pack(g, flat)
    table = Table(g)
    assert len(table.e) <= 64 and sorted(d['name'] for d in table.e) == sorted(want), 'the table lists every packed buffer once'
    assert g.D % 4 == 0 and g.P < 2 ** 31 and table.blocks < 2 ** 31
    for j, d in enumerate(table.e):
        assert find_entry(table, d['block0']) == j and find_entry(table, d['block0'] + (d['n'] + 255) // 256 - 1) == j, d['name']
        dst, src = entry_map(d)
        ref = want[d['name']]
        assert dst.size == ref.size, (d['name'], dst.size, ref.size)
        owners = np.bincount(dst.reshape(-1), minlength=ref.size)
        assert owners.min() == 1 and owners.max() == 1, f'{d["name"]}: a destination float without exactly one owner'
        assert src.max() < g.P and src.min() >= -1, d['name']
        got = np.zeros(ref.size)
        got[dst.reshape(-1)] = np.where(src.reshape(-1) >= 0, flat[np.maximum(src.reshape(-1), 0)], 0.0)
        assert np.array_equal(got, ref), f'{d["name"]} at {C} x {R} x {R}: the map does not invert the host packer'
        if d['swizzle']:    # a wave's 64 owners read eight 128-byte row segments and write eight 128-byte segments
            s0 = src[:64, 0]
            assert len(set(((s0 - d['src']) // 32).tolist())) == 8 and len(set((dst[:64, 0] // 32).tolist())) == 8, d['name']
    return g.P, len(table.e), table.blocks


def main():
    for C in (1, 2, 3):
        for R in RES:
            P, n, blocks = check(C, R)
            print(f'{C} x {R:3d} x {R:3d}: {P:9d} parameters, {n} entries, {blocks} workgroups: every map inverts its packer')
    return 0


if __name__ == '__main__':
    sys.exit(main())
