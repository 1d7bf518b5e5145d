"""The scripted synthetic search of the diverse step tests: `lp + cum` rows made up per step with what the rules
must get right planted into them, run through tests/diverse_ref.py.  tests/test_diverse_ref.py asserts (without a GPU)
that every planted event occurs; tests/test_gpu_beam_diverse.py feeds the same lists to `vs_beam_diverse_step`."""
import numpy as np

import beam_step_ref
import diverse_ref as DR

BSZ, BEAM, V, MAX_LEN, PAD, EOS = 5, 4, 50, 9, 49, 48
STEP_CASES = {"G2": dict(groups=2, lam=0.5), "G4": dict(groups=4, lam=0.5), "siblings": dict(rate=0.5)}


def _rows(rs, st, step):
    """fp32 `lp + cum` [bsz*beam, V] of one step."""
    rows = BSZ * BEAM
    x = np.log(rs.rand(rows, V)).astype(np.float32)
    if step:
        x = (x + st["sc"][:, step - 1][:, None]).astype(np.float32)
    x[:, EOS] -= 3.0
    for s in range(BSZ):
        r0 = s * BEAM
        srt = np.sort(x[r0: r0 + BEAM], axis=1)
        # one token on top of every row of the sentence, 0.2 above the row's runner-up: the groups' first choices
        # coincide and the penalty (0.5) moves the later groups to another token
        t = int(rs.randint(0, V - 2))
        x[r0: r0 + BEAM, t] = srt[:, -1] + np.float32(0.2)
        if step in (4, 6) and s == 2:
            # exact ties across two beams of one group (beams 0 and 2 share a group for G = 1, 2), entry by entry at
            # equal ranks: beam 2's row is beam 0's, one token to the right
            x[r0 + 2] = np.roll(x[r0], 1)
        if rs.rand() < 0.6:  # eos near the top of one row: inside or beyond the first `beam` candidates
            b = int(rs.randint(0, BEAM))
            r = int(rs.randint(1, 7))  # between the row's r-th and r+1-th best
            x[r0 + b, EOS] = (srt[b, -r] + srt[b, -r - 1]) / np.float32(2)
    if step == 1:  # a forced token: one finite entry per row of sentence 1, the groups fill up with -inf candidates
        keep = x[BEAM: 2 * BEAM, 7].copy()
        x[BEAM: 2 * BEAM] = -np.inf
        x[BEAM: 2 * BEAM, 7] = keep
    if step == 2:  # eos far on top of every row of sentence 0: it finishes here and idles from step 3 on
        x[:BEAM, EOS] = x[:BEAM].max(1) + np.float32(5.0)
    x[:, PAD] = -np.inf
    if step == MAX_LEN:
        x[:, :EOS] = -np.inf
        x[:, EOS + 1:] = -np.inf
    return x


def run_scripted(case, seed=3, on_step=None):
    """(counters, final state, gaps) of a case (a name of STEP_CASES, or a dict like its values).
    on_step(step, st, row_val, row_idx, new, reorder) sees every step."""
    case = STEP_CASES[case] if isinstance(case, str) else case
    rs = np.random.RandomState(seed)
    st = beam_step_ref.new_state(BSZ, BEAM, MAX_LEN, PAD, EOS, anc_ld=MAX_LEN + 2)
    cnt, gaps = DR.new_counters(), []
    for step in range(MAX_LEN + 1):
        rv, ri = beam_step_ref.row_lists(_rows(rs, st, step), None, 2 * BEAM)
        if step == 3:
            # With 2*beam candidates a search never sets cands_to_ignore itself (a sentence has at most `beam` eos
            # candidates, and `beam` of them in front finish it), so the flag is planted: beam 1 of sentence 3
            st = dict(st, ignore=st["ignore"].copy())
            st["ignore"][3, 1] = 1
        if case.get("rate") is not None:
            new, reorder = DR.sibling_step(st, rv, ri, step, V, EOS, MAX_LEN, case["rate"], counters=cnt, gaps=gaps)
        else:
            new, reorder = DR.group_step(st, rv, ri, step, V, EOS, MAX_LEN, case["groups"], case["lam"],
                                         counters=cnt, gaps=gaps)
        if on_step is not None:
            on_step(step, st, rv, ri, new, reorder)
        st = new
        if st["remaining"][0] == 0:
            break
    return cnt, st, gaps
