"""The host arithmetic of the feature-network kernels restated in plain Python: which template arm a shape is
dispatched to (LSTM_DISPATCH of bcnf_lstm.hip; ATTN_DISPATCH and LN_DISPATCH of bcnf_attn.hip; CONV_K_DISPATCH of
bcnf_conv.hip) and what the host planners make of it (ln_plan; wgrad_plan and tile_plan of bcnf_conv.hip). No GPU and
no library: tests/test_feature_plans_cpu.py holds the restatement to the library's byte counts and holds the GPU
files' case lists to the arm sets and the branch registry below.

A new dispatch arm or plan branch is registered HERE -- in the arm set, or as an entry of *_BRANCHES -- and the census
then fails until a case of the GPU lists reaches it."""
from collections import namedtuple

# ------------------------------------------------------------------------------------------ LSTM (bcnf_lstm.hip)
LSTM_ARMS = frozenset(range(16, 129, 16))


def lstm_arm(H):
    """k_lstm_fwd<H> / k_lstm_bwd<H>, or None where the library refuses."""
    return H if H in LSTM_ARMS else None


# label -> predicate over a (B, S, H, dirs) case
LSTM_BRANCHES = {
    "one step in both directions": lambda c: c[1] == 1 and c[3] == 2,
}

# ------------------------------------------------------------------------------------------ attention, LayerNorm
ATTN_ARMS = frozenset((sb, hb) for sb in (32, 64) for hb in (8, 16, 32, 64))
LN_ARMS = frozenset((1, 2, 4, 8, 16))
LN_MAX_D, LN_MAX_WG, LN_MIN_RPW = 1024, 1024, 8


def attn_arm(S, hd):
    """(SB, HDB) of k_attn_fwd / k_attn_bwd, or None where the library refuses."""
    if not (1 <= S <= 64 and 1 <= hd <= 64):
        return None
    return (32 if S <= 32 else 64, 8 if hd <= 8 else 16 if hd <= 16 else 32 if hd <= 32 else 64)


# label -> predicate over a (B, S, heads, hd) case
ATTN_BRANCHES = {
    "head_dim 1": lambda c: c[3] == 1,
    "the last S of the two-slot form": lambda c: c[1] == 32,
    "the first head_dim past 8": lambda c: c[3] == 9,
    "the first head_dim of <32,64>": lambda c: c[1] <= 32 and c[3] == 33,
    "<64,16> at its upper edge": lambda c: c[1] == 64 and c[3] == 16,
}


def ln_arm(d):
    """T of k_add_ln_fwd<T> / k_add_ln_bwd<T>: elements per lane of a row, or None where the library refuses."""
    if not 1 <= d <= LN_MAX_D:
        return None
    return 1 if d <= 64 else 2 if d <= 128 else 4 if d <= 256 else 8 if d <= 512 else 16


def ln_plan(rows, d):
    """(rpw, nwg) of the backward: rows per workgroup and workgroups (= partials of dgamma | dbeta)."""
    assert rows >= 1 and ln_arm(d) is not None
    nwg = min((rows + LN_MIN_RPW - 1) // LN_MIN_RPW, LN_MAX_WG)
    rpw = (rows + nwg - 1) // nwg
    return rpw, (rows + rpw - 1) // rpw


def ln_work_bytes(rows, d):
    return ln_plan(rows, d)[1] * 2 * d * 4


# label -> predicate over a (rows, d) pair
LN_BRANCHES = {
    "the first d of T = 2": lambda c: c[1] == 65,
    "the first d of T = 8": lambda c: c[1] == 257,
    "T = 8 with whole registers past the row and one partly inside": lambda c: ln_arm(c[1]) == 8 and c[1] % 64 > 1,
    "the last d of T = 8": lambda c: c[1] == 512,
    "several workgroups of fewer than LN_MIN_RPW rows, no multiple of the four waves":
        lambda c: c[0] > ln_plan(*c)[0] and ln_plan(*c)[0] < LN_MIN_RPW and ln_plan(*c)[0] % 4 != 0,
    "the workgroup cap at T = 1": lambda c: ln_plan(*c)[0] > LN_MIN_RPW and ln_arm(c[1]) == 1,
    "the workgroup cap at T = 2": lambda c: ln_plan(*c)[0] > LN_MIN_RPW and ln_arm(c[1]) == 2,
}

# ------------------------------------------------------------------------------------------ convolution (bcnf_conv.hip)
CONV_K_ARMS = frozenset(range(1, 9))
CWG, OCB, WCB = 256, 8, 4
TILE_LDS_BYTES, WGRAD_LDS_BYTES, WGRAD_MAX_WG = 32 * 1024, 64 * 1024, 512


def conv_k_arm(K):
    return K if K in CONV_K_ARMS else None


def conv_dims(case):
    """(HC, WC, HP, WP): the convolution output and the pooled output of a (N, c_in, H, W, c_out, K, pad_h, pad_w)."""
    _, _, H, W, _, K, ph, pw = case
    hc, wc = H + 2 * ph - K + 1, W + 2 * pw - K + 1
    return hc, wc, hc // 2, wc // 2


WgradPlan = namedtuple("WgradPlan", "COP GW GWC BR YS tpp passes nwg P chunks ragged bands shrinks")


def conv_wgrad_plan(case):
    """wgrad_plan. `chunks` x chunks of GWC columns cover GW, the last one `ragged` = GW % GWC wide where that is not
    zero; `bands` row bands of BR rows cover 2 HP; `shrinks` is the sequence of branches the fitting loop took:
    "br" (keep the row slices busy), "gwc" (down to 4 K columns), "br4", "gwc_k" (the GWC > K branch), "br1"."""
    N, CI, _, _, CO, K, _, _ = case
    _, _, HP, WP = conv_dims(case)
    COP = (CO + WCB - 1) // WCB * WCB
    GW = (2 * WP + K - 1) // K * K
    gwc = GW
    ntasks = (COP // WCB) * CI * K
    tpp = min(ntasks, CWG)
    ys_want = CWG // tpp
    br = min(2 * HP, 16)

    def nbytes(b, g):
        return (COP * b * g + CI * (b + K - 1) * (g + K)) * 4

    def halved(g):
        return ((g // K + 1) // 2) * K
    shrinks = []
    while nbytes(br, gwc) > WGRAD_LDS_BYTES:
        if br > max(ys_want, 4):
            br, step = (br + 1) // 2, "br"
        elif gwc > 4 * K:
            gwc, step = halved(gwc), "gwc"
        elif br > 4:
            br, step = (br + 1) // 2, "br4"
        elif gwc > K:
            gwc, step = halved(gwc), "gwc_k"
        elif br > 1:
            br, step = (br + 1) // 2, "br1"
        else:
            break
        shrinks.append(step)
    return WgradPlan(COP=COP, GW=GW, GWC=gwc, BR=br, YS=min(ys_want, br), tpp=tpp, passes=(ntasks + tpp - 1) // tpp,
                     nwg=min(N, WGRAD_MAX_WG), P=COP * CI * K * K + COP, chunks=(GW + gwc - 1) // gwc,
                     ragged=GW % gwc, bands=(2 * HP + br - 1) // br, shrinks=tuple(shrinks))


def conv_work_bytes(case):
    p = conv_wgrad_plan(case)
    return p.nwg * p.YS * p.P * 4


TilePlan = namedtuple("TilePlan", "TH TW tiles_x tiles_y cib rounds")


def conv_tile_plan(np_y, np_x, K, IC):
    """tile_plan for np_y x np_x thread patches over IC staged channels: the (TH, TW) with the smallest padded area,
    the larger workgroup on a tie; `rounds` staging rounds of `cib` channels."""
    best = None
    for tl in (3, 4, 5):
        th = 2
        while th <= 32:
            tw = 1 << tl
            nt = th * tw
            if 64 <= nt <= CWG:
                area = (np_y + th - 1) // th * th * ((np_x + tw - 1) // tw) * tw
                if best is None or area < best[0] or (area == best[0] and nt > best[1] * best[2]):
                    best = (area, th, tw)
            th *= 2
    _, TH, TW = best
    plane_bytes = (2 * TH + K - 1) * (2 * TW + K - (K & 1)) * 4
    cib = max(1, min(TILE_LDS_BYTES // plane_bytes, IC))
    return TilePlan(TH=TH, TW=TW, tiles_x=(np_x + TW - 1) // TW, tiles_y=(np_y + TH - 1) // TH, cib=cib,
                    rounds=(IC + cib - 1) // cib)


def conv_forward_tiles(case):
    """tile_plan of k_conv_tile<K, false>: a thread per pooled pixel, c_in staged channels."""
    _, CI, _, _, _, K, _, _ = case
    _, _, HP, WP = conv_dims(case)
    return conv_tile_plan(HP, WP, K, CI)


def conv_backward_tiles(case):
    """tile_plan of k_conv_tile<K, true>: a thread per 2 x 2 patch of dx, c_out staged channels."""
    _, _, H, W, CO, K, _, _ = case
    return conv_tile_plan((H + 1) // 2, (W + 1) // 2, K, CO)


def _fields(plan, **want):
    return all(getattr(plan, k) == v for k, v in want.items())


# The (N, c_in, H, W, c_out, K, pad_h, pad_w) that reaches a branch of wgrad_plan / k_conv_wgrad / k_conv_tile, and the
# predicate over (case, wgrad plan, forward tile plan, backward tile plan) that says it does.
ConvBranch = namedtuple("ConvBranch", "case reaches")
CONV_BRANCHES = {
    "K = 2 over several input channels, c_out no multiple of WCB": ConvBranch(
        (2, 3, 9, 12, 5, 2, 1, 0), lambda c, w, f, b: c[5] == 2 and c[1] > 1 and c[4] % WCB != 0),
    "K = 7 with pad_w = K - 1": ConvBranch(
        (2, 4, 9, 14, 6, 7, 3, 6), lambda c, w, f, b: c[5] == 7 and c[7] == 6),
    "a workgroup's n += nwg loop takes a second and a third image": ConvBranch(
        (1025, 1, 4, 5, 3, 2, 0, 1), lambda c, w, f, b: w.nwg == 512 and c[0] == 2 * w.nwg + 1),
    "four x chunks with a ragged last one, two bands, three passes; forward tiles x rounds": ConvBranch(
        (1, 32, 8, 160, 32, 3, 1, 1),
        lambda c, w, f, b: _fields(w, GW=162, GWC=42, chunks=4, ragged=36, BR=4, bands=2, passes=3)
        and (f.tiles_y, f.tiles_x, f.rounds) == (1, 5, 2)),
    "an odd chunk width: a pooling window straddles two x chunks": ConvBranch(
        (1, 32, 8, 50, 32, 5, 2, 2),
        lambda c, w, f, b: _fields(w, GWC=25, chunks=2, passes=5) and f.rounds == 4),
    "an odd band height: a pooling window straddles two row bands": ConvBranch(
        (1, 32, 15, 16, 32, 3, 1, 1), lambda c, w, f, b: _fields(w, BR=7, bands=2, chunks=1)),
    "the GWC > K halving branch": ConvBranch(
        (1, 32, 40, 24, 32, 8, 7, 7),
        lambda c, w, f, b: w.shrinks[-1] == "gwc_k" and _fields(w, GWC=16, BR=4, bands=12, passes=8)),
    "K = 7 at scale: chunks, bands, passes, tiles and rounds at once": ConvBranch(
        (1, 20, 37, 150, 32, 7, 3, 3),
        lambda c, w, f, b: _fields(w, GW=154, GWC=42, chunks=4, ragged=28, bands=9, passes=5)
        and (f.tiles_y, f.tiles_x) == (5, 5) and (b.tiles_y, b.tiles_x) == (5, 5)
        and f.rounds in (2, 3) and b.rounds in (2, 3)),
}
