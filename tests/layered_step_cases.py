"""Case tables of the layered rollout's step entries -- mrl_rollout_reset_rows, mrl_rollout_obs,
mrl_rollout_act, mrl_rollout_act_head and mrl_rollout_act_head_bf16 (csrc/rollout_layered.hip,
rollout_layered_kernels.h, rollout_layered_eval.hip; the record merge of rollout_device.h) --
and ``branches(case)``, which restates from the case alone which kernel branch it reaches.
tests/layered_step_np.py holds the operands, references and wrong twins; test_layered_step_host.py
is the CPU half, test_gpu_layered_step.py the GPU half."""
from collections import namedtuple

# env -> (obs dims O, action dims A); D = O + 1 columns (the reward last) meet LCOLS = 32
ENVS = {"CartPole-v0": (4, 2), "Hopper-v2": (11, 3), "HalfCheetah-v2": (17, 6), "Humanoid-v2": (376, 17)}
BLOCK = 64   # ENVS_PER_BLOCK: envs per record block
LCOLS = 32   # columns per chunk of the obs and partials kernels
LREC = 16    # record blocks per chunk of merge_records_column
A_HEAD = 17  # HM_ACT: the fused head is the Humanoid step's

# ------------------------------------------------------------------ 1. the fused head
# mode: f32 rows / f32 rows rounded to bf16 in the kernel (bf = 1) / bf16 rows given as bits.
# align "mis" (n_hidden 256 and 512 only) runs the aligned call, the head kernel offset by one
# float and the hidden rows offset by 8 bytes in one case: the last two take the strided route.
HeadCase = namedtuple("HeadCase", "nh mode align E wpb ev t")
MODES = ("f32", "bf", "b16")
HEAD_E = (1, 3, 4, 5, 130)


def _head_cases():
    out = []
    for nh in (512, 256):  # runs<8>, runs<4>: never cut
        for mode in MODES:
            for i, E in enumerate(HEAD_E):
                for wpb in (1, 4):
                    out.append(HeadCase(nh, mode, "al", E, wpb, 0, (i + wpb) % 2))
            out.append(HeadCase(nh, mode, "mis", 5, 4, 0, 0))
            out.append(HeadCase(nh, mode, "mis", 3, 1, 0, 1))
    for i, nh in enumerate((128, 64, 200, 30, 1)):  # the lane loop: E and WPB cut first
        for mode in MODES:
            out.append(HeadCase(nh, mode, "al", 5, 4, 0, i % 2))
            out.append(HeadCase(nh, mode, "al", 130 if nh in (200, 30) else 3, 1, 0, (i + 1) % 2))
    for nh, mode in ((512, "f32"), (256, "b16"), (200, "f32")):  # the second instantiation
        out.append(HeadCase(nh, mode, "al", 5, 4, 1, 0))
        out.append(HeadCase(nh, mode, "al", 3, 1, 1, 1))
    return out


HEAD = _head_cases()
HEAD_T = 2  # horizon of the head cases: t = 0 and t = horizon - 1


def head_route(nh, aligned):
    if aligned and nh == 512:
        return "runs8"
    if aligned and nh == 256:
        return "runs4"
    return "strided"


def head_variants(c):
    """(name, head-kernel offset in floats, hidden-row offset in bytes) of the calls a case makes."""
    if c.align == "al":
        return [("al", 0, 0)]
    return [("al", 0, 0), ("woff", 1, 0), ("hoff", 0, 8)]


def _head_branches(c):
    b = set()
    for name, woff, hoff in head_variants(c):
        r = head_route(c.nh, woff == 0 and hoff == 0)
        b.add("head:%s:%s" % (r, c.mode))
        if name != "al":
            b.add("head:fallback_" + name)
        if r == "runs4" and c.mode == "b16":
            b.add("head:uint2_tail")
        if r == "strided":
            b.add("head:whole_strides" if c.nh % 64 == 0 else "head:ragged_stride" if c.nh > 64 else "head:idle_lanes")
            if c.nh == 1:
                b.add("head:one_unit")
    b.add("head:wpb%d" % c.wpb)
    if c.wpb == 4 and c.E % 4:
        b.add("head:ragged_block")  # waves past E load env E - 1 and store nothing
    if c.wpb == 4 and c.E > 4:
        b.add("head:blocks>1")
    if c.ev:
        b.add("head:eval:%s:%s" % (head_route(c.nh, True), c.mode))
    b.add("head:t%d" % c.t)
    return b


# ------------------------------------------------------------------ 2. mrl_rollout_obs
# state: the running stat the merge starts from -- "empty" (n = 0), "running" (earlier batches),
# "single" (n = 1: the evaluation filter's n < 2).  Every case carries a constant column
# (column 1 where O >= 2: S = 0, denominator 1e-8), values that clip at +5 and (E > 1) -5, a
# reward count of 0 at t = 0, and from three blocks up a record block of count 0 mid-list.
ObsCase = namedtuple("ObsCase", "env E t state filt twin ev")
OBS_T = 5  # horizon: t = 0, 1 and 4 cover both buffer parities
OBS_E = (1, 63, 64, 65, 130)
OBS_E_BIG = (1024, 1025, 2049)  # nb = 16, 17 (one-env last block), 33 (one-block last chunk)


def _obs_cases():
    out, i = [], 0
    for env in ENVS:
        for E in OBS_E + (OBS_E_BIG if env in ("CartPole-v0", "Humanoid-v2") else ()):
            t = (0, 1, OBS_T - 1)[i % 3]
            out.append(ObsCase(env, E, t, ("running", "empty")[(i // 3) % 2], 0 if i % 5 == 3 else 1, i % 2, 0))
            i += 1
        out.append(ObsCase(env, 1, 1, "empty", 1, 1, 0))  # n = 1 after the merge: var = M * M
    # the chunked merge from both parities, and from an empty state
    out.append(ObsCase("CartPole-v0", 1025, 0, "empty", 1, 1, 0))
    out.append(ObsCase("Humanoid-v2", 2049, 1, "running", 1, 0, 0))
    for env in ("CartPole-v0", "Humanoid-v2"):  # the frozen filter
        out.append(ObsCase(env, 65, 0, "running", 1, 1, 1))
        out.append(ObsCase(env, 130, 1, "single", 1, 0, 1))
        out.append(ObsCase(env, 63, OBS_T - 1, "empty", 1, 0, 1))
    out.append(ObsCase("Hopper-v2", 65, 1, "running", 0, 1, 1))
    return out


OBS = _obs_cases()


def n_blocks(E):
    return (E + BLOCK - 1) // BLOCK


def zero_block(E):
    """The record block of count 0 of an obs case, or None below three blocks."""
    nb = n_blocks(E)
    return nb // 2 if nb >= 3 else None


def const_column(env):
    return 1 if ENVS[env][0] >= 2 else None


def _geometry_branches(pre, env, E):
    O = ENVS[env][0]
    D = O + 1
    nb = n_blocks(E)
    last = E - BLOCK * (nb - 1)
    b = {pre + ("nvalid1" if last == 1 else "nvalid64" if last == 64 else "nvalid_ragged")}
    b.add(pre + ("blocks1" if nb == 1 else "blocks>1"))
    b.add(pre + ("col_chunks1" if D <= LCOLS else "col_chunks>1"))
    if O % LCOLS:
        b.add(pre + "reward_chunk_with_obs")  # the chunk of column O holds obs columns too
    if D % LCOLS:
        b.add(pre + "ragged_last_chunk")
    return b


def _obs_branches(c):
    nb = n_blocks(c.E)
    b = _geometry_branches("obs:", c.env, c.E)
    b.add("obs:filter%d" % c.filt)
    b.add("obs:twin" if c.twin else "obs:notwin")
    if c.twin and ENVS[c.env][0] % 8:
        b.add("obs:twin_padded")
    b.add("obs:t_last" if c.t == OBS_T - 1 else "obs:t%d" % c.t)
    if c.ev:
        b.add("obs:eval")
        b.add("obs:eval:n>=2" if c.state == "running" else "obs:eval:n<2")
        return b
    b.add("obs:parity%d" % (c.t & 1))
    b.add("merge:nb<=16" if nb <= LREC else "merge:nb>16")
    if nb == LREC:
        b.add("merge:nb==16")
    if nb > LREC and nb % LREC:
        b.add("merge:partial_last_chunk")
    if nb > LREC and nb % LREC == 1:
        b.add("merge:one_block_last_chunk")
    b.add("merge:state_" + c.state)
    if c.state == "empty" and c.E == 1:
        b.add("obs:var_n<=1")
    if const_column(c.env) is not None:
        b.add("obs:zero_variance")
    if c.t == 0:
        b.add("merge:zero_count_reward")
    if zero_block(c.E) is not None:
        b.add("merge:zero_count_block")
    b.add("obs:clip")
    return b


# ------------------------------------------------------------------ 3. the records
# mrl_rollout_reset_rows' partials (half 0, reward count 0); ``act``: one mrl_rollout_act on top
# (half 1, reward count nvalid)
RecCase = namedtuple("RecCase", "env E act")
REC = [RecCase(env, E, int(E == 65)) for env in ENVS for E in (1, 64, 65, 130)]


def _rec_branches(c):
    b = _geometry_branches("rec:", c.env, c.E)
    b.add("rec:with_reward" if c.act else "rec:reset")
    if c.E == 1:
        b.add("rec:m2_exact_zero")
    return b


# ------------------------------------------------------------------ 4. mrl_rollout_act, a thread per env
ActCase = namedtuple("ActCase", "env E")
ACT = [ActCase(env, E) for env in ("CartPole-v0", "Hopper-v2") for E in (1, 63, 64, 65)]


def _act_branches(c):
    b = {"act:categorical" if c.env == "CartPole-v0" else "act:gauss"}
    b.add("act:blocks1" if c.E <= 64 else "act:blocks>1")
    b.add("act:full_block" if c.E % 64 == 0 else "act:ragged_block")
    return b


def branches(c):
    return {HeadCase: _head_branches, ObsCase: _obs_branches, RecCase: _rec_branches, ActCase: _act_branches}[type(c)](c)


def case_id(c):
    return "-".join(str(v) for v in c)
