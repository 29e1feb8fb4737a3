"""
The paired K halves of the fused kernel's bf16 sweeps (vn_fused16_common.h: stage_split_hidden<L, FOLD13>, khalf_pack, five_khalf,
three_khalf), emulated in numpy from the image up: the 20-block image of one 50-wide layer is staged as the kernel stages it (out-fold
rows, in-fold slots, the forward operands kept in the edge halves of the piece-1 and piece-2 entries, no in-fold in row tile 3), both
sweeps read their fragments from it (row entries forward, transposed reads in the sweep back), and every 16x16x32 MFMA is a sum over
its 32 K slots of (A slot) x (B slot).  Every slot carries, beside its bf16 value, what it is: (in-feature, out-feature, piece) for a
weight, (feature, piece) for a value -- so the test sees which piece products each (in, out) pair receives, and how often:

  * a weight slot only ever meets the value of its own in- (forward) or out-feature (sweep back), and lands in its own row;
  * every one of the six products hh, hm, mh, hl, lh, mm of every (in, out) pair occurs exactly once, in 11 MFMAs per row tile and
    stream (6 + 5) and 6 for the folded tile; the three small products ml, lm, ll occur at most once (folded rows: all nine);
  * the corner of the folded tile (features 48, 49 on both sides) is not counted twice;
  * numerically, result - six-term result <= 2^-24 * sum |w x|.
Widths 50, 49, 48 and 33 on either side.  The values of padding features below k-step 13 (50, 51; a narrower layer's) are NOT zero, as
in the kernel (the activation of a zero pre-activation): only the zero weights keep them out.
"""
import numpy as np
import pytest

KS = 13
SIX = [(0, 0), (0, 1), (1, 0), (0, 2), (2, 0), (1, 1)]                 # (weight piece, value piece)
SMALL = [(1, 2), (2, 1), (2, 2)]


def trunc_bf16(x):
    return (np.asarray(x, np.float32).view(np.uint32) & np.uint32(0xffff0000)).view(np.float32)


def split3(x):
    x = np.asarray(x, np.float32)
    h = trunc_bf16(x)
    r = x - h
    m = trunc_bf16(r)
    return [h, m, trunc_bf16(r - m)]


def vfeat(pos):
    return 4 * (4 * (pos >> 4) + (pos & 3)) + ((pos >> 2) & 3)


class Slots:
    """an array of K slots: bf16 value + tags; piece < 0 marks an exact zero"""

    def __init__(self, shape):
        self.v = np.zeros(shape, np.float64)
        self.fi = np.full(shape, -1)
        self.fo = np.full(shape, -1)
        self.pc = np.full(shape, -1)

    def take(self, idx):
        s = Slots(self.v[idx].shape)
        s.v, s.fi, s.fo, s.pc = self.v[idx].copy(), self.fi[idx].copy(), self.fo[idx].copy(), self.pc[idx].copy()
        return s

    def put(self, idx, o, oidx=slice(None)):
        self.v[idx], self.fi[idx], self.fo[idx], self.pc[idx] = o.v[oidx], o.fi[oidx], o.fo[oidx], o.pc[oidx]

    def zero(self, idx):
        self.v[idx], self.fi[idx], self.fo[idx], self.pc[idx] = 0.0, -1, -1, -1


def cat(a, b):
    s = Slots(a.v.shape[:-1] + (a.v.shape[-1] + b.v.shape[-1],))
    for n in ('v', 'fi', 'fo', 'pc'):
        setattr(s, n, np.concatenate([getattr(a, n), getattr(b, n)], axis=-1))
    return s


def stage_image(W, Hin, Hout):
    """stage_split_hidden<L, true> for one layer: {(piece, q, row tile): Slots[g, c, 8]}, 20 blocks"""
    P = split3(W)
    img = {}
    for q in range(2):
        for mt in range(4):
            e = [Slots((4, 16, 8)) for _ in range(3)]
            for g in range(4):
                for c in range(16):
                    fold_r = (c & 3) if mt == 3 else 0
                    ofold = fold_r in (1, 2)
                    fo = 48 + (c >> 2) if ofold else vfeat(16 * mt + c)
                    for j in range(8):
                        fi = 4 * (8 * q + j) + g
                        if fi < Hin and fo < Hout:
                            for p in range(3):
                                e[p].v[g, c, j], e[p].fi[g, c, j], e[p].fo[g, c, j], e[p].pc[g, c, j] = P[p][fi, fo], fi, fo, p
                    ix = (g, c)
                    if ofold:
                        e[0].put(ix, e[1 if fold_r == 1 else 2], ix)
                        e[1].zero(ix)
                        e[2].zero(ix)
                    elif q == 1 and mt != 3:
                        for p, slot in ((1, 5), (2, 6)):                 # in-fold: m-, l-piece of slot 4 into slots 5, 6
                            assert e[0].pc[g, c, slot] < 0
                            e[0].put((g, c, slot), e[p], (g, c, 4))
                        e[1].put((g, c, slice(4, 8)), e[1], (g, c, slice(0, 4)))      # [A1 | A1]
                        e[2].zero((g, c, slice(4, 8)))                                # [A2 | 0]
            img[(0, q, mt)] = e[0]
            if mt != 3:
                img[(1, q, mt)] = e[1]
                img[(2, q, mt)] = e[2]
    assert len(img) == 20
    return img


def value_operand(x, q):
    """plain B pieces of K fragment q: Slots[piece][g, 8]; k-steps >= 13 exact zeros"""
    X = split3(x)
    B = [Slots((4, 8)) for _ in range(3)]
    for p in range(3):
        for g in range(4):
            for j in range(8):
                k = 8 * q + j
                if k < KS:
                    B[p].v[g, j], B[p].fi[g, j], B[p].pc[g, j] = X[p][4 * k + g], 4 * k + g, p
    return B


def khalf_pack(B):
    lo, e4 = slice(0, 4), slice(4, 5)
    K0 = cat(B[0].take((slice(None), lo)), B[1].take((slice(None), lo)))
    Eh = Slots((4, 4))
    for s in range(3):
        Eh.put((slice(None), slice(s, s + 1)), B[0], (slice(None), e4))          # dup_lo16(h), h: slots 4, 5, 6
    K1 = cat(B[2].take((slice(None), lo)), Eh)
    Em = Slots((4, 4))
    for s in range(2):
        Em.put((slice(None), slice(s, s + 1)), B[1], (slice(None), e4))          # dup_lo16(m), 0
    El = Slots((4, 4))
    El.put((slice(None), slice(0, 1)), B[2], (slice(None), e4))
    return [K0, K1, cat(Em, El)]


class Sweep:
    def __init__(self, back):
        self.back = back
        self.count = np.zeros((64, 64, 3, 3), int)           # [in-feature, out-feature, weight piece, value piece]
        self.acc = np.zeros((4, 16))                         # [row tile, row]: one point (column) of the accumulators
        self.n_mfma = np.zeros(4, int)

    def mfma(self, A, B, mt):
        """A: Slots[g, c, 32-slot half pair (8)], B: Slots[g, 8]; rows c of row tile mt"""
        self.n_mfma[mt] += 1
        bv, bf, bp = B.v[:, None, :], B.fi[:, None, :], B.pc[:, None, :]
        live = (A.pc >= 0) & (bp >= 0)
        feat = A.fo if self.back else A.fi                   # the contraction index of a weight slot
        assert np.all((feat == bf)[live]), 'a weight slot against the value of another feature'
        rows = A.fi if self.back else A.fo                   # where it must land
        for c in range(16):
            want = 48 + (c >> 2) if (mt == 3 and (c & 3) in (1, 2)) else vfeat(16 * mt + c)
            r = rows[:, c, :][live[:, c, :]]
            assert np.all(r == want), 'a weight slot in the row of another feature'
        g, c, j = np.nonzero(live)
        np.add.at(self.count, (A.fi[g, c, j], A.fo[g, c, j], A.pc[g, c, j], np.broadcast_to(bp, A.pc.shape)[g, c, j]), 1)
        self.acc[mt] += (A.v * bv).sum(axis=(0, 2))

    def result(self):
        out = np.zeros(64)
        t = self.acc.copy()
        t[3, 0::4] = (t[3, 0::4] + t[3, 1::4]) + t[3, 2::4]                       # fold_rows
        for mt in range(4):
            for c in range(16):
                if mt == 3 and (c & 3):
                    continue
                out[vfeat(16 * mt + c)] = t[mt, c]
        return out


def frag_row(img, p, q, mt):
    return img[(p, q, mt)]


def frag_tr_half(img, p, mo, mt):
    """ds_read_b64_tr_b16 of out row tile mo for in row tile mt: Slots[g, c', 4]"""
    blk = img[(p, mt >> 1, mo)]
    h = Slots((4, 16, 4))
    for g in range(4):
        for c in range(16):
            for r in range(4):
                h.put((g, c, r), blk, ((c >> 2) & 3, 4 * g + r, 4 * (mt & 1) + (c & 3)))
    return h


def zeros_half():
    return Slots((4, 16, 4))


def sweep(img, x, back):
    s = Sweep(back)
    six = [(1, 1), (2, 0), (0, 2), (1, 0), (0, 1), (0, 0)]
    B = value_operand(x, 0)
    for mt in range(4):
        if back:
            A = [cat(frag_tr_half(img, p, 0, mt), frag_tr_half(img, p, 1, mt)) for p in range(3 if mt < 3 else 1)]
        else:
            A = [frag_row(img, p, 0, mt) for p in range(3 if mt < 3 else 1)]
        if mt == 3:
            for p in (2, 1, 0):
                s.mfma(A[0], B[p], mt)                                             # three_folded
        else:
            for pa, pb in six:
                s.mfma(A[pa], B[pb], mt)
    K = khalf_pack(value_operand(x, 1))
    lo, hi = (Ellipsis, slice(0, 4)), (Ellipsis, slice(4, 8))
    for mt in (3, 0, 1, 2):
        if back:
            T0, E0 = frag_tr_half(img, 0, 2, mt), frag_tr_half(img, 0, 3, mt)
        else:
            Ad = frag_row(img, 0, 1, mt)
            T0, E0 = Ad.take(lo), Ad.take(hi)
        if mt == 3:                                                                # three_khalf
            s.mfma(cat(E0, E0), K[2], mt)
            s.mfma(cat(T0, E0), K[1], mt)
            s.mfma(cat(T0, T0), K[0], mt)
            continue
        if back:
            T1, T2 = frag_tr_half(img, 1, 2, mt), frag_tr_half(img, 2, 2, mt)
            Ab, Ac = cat(T1, T1), cat(T2, zeros_half())
        else:
            Ab, Ac = frag_row(img, 1, 1, mt), frag_row(img, 2, 1, mt)
        s.mfma(Ac, K[0], mt)                                                       # five_khalf
        s.mfma(Ab, K[0], mt)
        s.mfma(cat(E0, E0), K[2], mt)
        s.mfma(cat(T0, E0), K[1], mt)
        s.mfma(cat(T0, T0), K[0], mt)
    return s


@pytest.mark.parametrize('back', [False, True], ids=['forward', 'back'])
@pytest.mark.parametrize('Hin,Hout', [(50, 50), (49, 49), (48, 48), (33, 33), (50, 33), (33, 50), (49, 50), (48, 49)])
def test_khalf_products_once_and_close_to_six_terms(Hin, Hout, back):
    rng = np.random.default_rng(100 * Hin + Hout + (7 if back else 0))
    W = np.zeros((64, 64), np.float32)
    W[:Hin, :Hout] = (rng.standard_normal((Hin, Hout)) * 0.4).astype(np.float32)
    x = np.zeros(64, np.float32)
    x[:4 * KS] = rng.uniform(0.05, 1, 4 * KS).astype(np.float32) * rng.choice([-1, 1], 4 * KS)    # padding values are NOT zero
    s = sweep(stage_image(W, Hin, Hout), x, back)
    assert list(s.n_mfma) == [11, 11, 11, 6]
    n_c, n_o = (Hout, Hin) if back else (Hin, Hout)                    # contraction side, result side
    Wp = [p.astype(np.float64) for p in split3(W)]
    Xp = [p.astype(np.float64) for p in split3(x)]
    for fi in range(64):
        for fo in range(64):
            cnt = s.count[fi, fo]
            if fi >= Hin or fo >= Hout:
                assert cnt.sum() == 0
                continue
            for t in SIX:
                assert cnt[t] == 1, ('six products exactly once', fi, fo, t, cnt)
            for t in SMALL:
                assert cnt[t] <= 1, ('small product twice', fi, fo, t, cnt)
            folded_row = (fi if back else fo) >= 48
            assert cnt.sum() == (9 if folded_row and not (back and fo >= 48) else 6), (fi, fo, cnt)
    # the corner: both features on the edge k-step -- nine products forward (rows h, m, l against E_h, E_m, E_l), six in the sweep back
    if Hin > 48 and Hout > 48:
        assert s.count[48, 48].sum() == (6 if back else 9) and s.count[48, 48].max() == 1
    got = s.result()
    worst = 0.0
    for r in range(n_o):
        w = W[r, :] if back else W[:, r]
        six_term = sum((Wp[a][r, :] if back else Wp[a][:, r])[:n_c] @ Xp[b][:n_c] for a, b in SIX)
        scale = np.abs(w[:n_c].astype(np.float64) * x[:n_c]).sum()
        assert abs(got[r] - six_term) <= 2.0 ** -24 * scale, (r, got[r], six_term, scale)
        worst = max(worst, abs(got[r] - six_term) / scale)
    assert np.all(got[n_o:] == 0)
    print('K halves - six-term: %.2e of sum |w x| (%s, %d -> %d)' % (worst, 'back' if back else 'forward', Hin, Hout))


def test_in_fold_on_the_corner_would_count_twice():
    """the guard of stage_split_hidden: with the in-fold also on row tile 3 (the image of the parent commit), E_h and E_m reach the
    corner's m- and l-pieces a second time"""
    rng = np.random.default_rng(5)
    W = (rng.standard_normal((64, 64)) * 0.4).astype(np.float32)
    W[50:], W[:, 50:] = 0, 0
    x = rng.uniform(0.05, 1, 64).astype(np.float32)
    img = stage_image(W, 50, 50)
    e = img[(0, 1, 3)]
    P = split3(W)
    for g in range(2):
        for c in (0, 4):
            fi, fo = 48 + g, 48 + (c >> 2)
            for p, slot in ((1, 5), (2, 6)):
                e.v[g, c, slot], e.fi[g, c, slot], e.fo[g, c, slot], e.pc[g, c, slot] = P[p][fi, fo], fi, fo, p
    s = sweep(img, x, False)
    assert s.count[48, 48].max() == 2
