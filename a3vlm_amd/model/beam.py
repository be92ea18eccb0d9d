"""Beam search on the ragged decode path (``MetaModel.beam_search``; no reference counterpart; opt-in).

Groups of K = ``num_beams`` consecutive KV-cache rows, one prompt per group.  The prompt is prefilled ONCE, on the group's leader row;
the siblings read its keys from that row (``share_prefix``) and start from its logits.  Per step, with no host read:

    a3v_logits_prepare (lse of the raw rows) -> a3v_beam_select (the best 2K of the K * V candidates of a group)
    -> a3v_beam_advance (HF's BeamSearchScorer walk: finished hypotheses into the group's pool, the next K live beams, their token
    rows) -> a3v_kv_permute_tails (the generated keys of a parent into its children's cache rows) -> forward_inference_rows.

``tests/beam_ref.py`` restates select and advance bit for bit and is the contract of the semantics.  Scores are sums of the RAW
log-probabilities of the unconstrained model, also under a constraint.

Cost: the permute moves the generated tail of every re-parented beam in every layer, so a step's extra traffic grows linearly with
the answer's length (7B: 0.524 MB per copied position and row).  Beam search is for the short structured answers of this task, not
for long free text."""
from __future__ import annotations

from typing import Iterable, List, Optional

import torch

from .. import ops
from . import constrain

MAX_BEAMS = 8


def len_div_table(n: int, length_penalty: float) -> torch.Tensor:
    """len_div[j] = fp32(max(j, 1) ** length_penalty), computed in fp64 on the host (no device powf)."""
    return torch.tensor([float(max(j, 1)) ** float(length_penalty) for j in range(n)], dtype=torch.float64).to(torch.float32)


def check_beam_args(num_beams, batch_rows, num_return_sequences=1, *, temperature: float = 0.0, repetition_penalty: float = 1.0,
                    additional_stop_symbols: Iterable[str] = (), lookup=None, who: str = "beam_search") -> int:
    """Every refusal of beam search that needs no model: a ``ValueError`` before any device use, naming the way out."""
    K = int(num_beams)
    if K < 1 or K > MAX_BEAMS:
        raise ValueError(f"{who}: num_beams = {K}; 1 .. {MAX_BEAMS} (the select kernel keeps 2 * num_beams candidates per thread in "
                         f"registers): use num_beams <= {MAX_BEAMS}")
    if K > int(batch_rows):
        raise ValueError(f"{who}: num_beams = {K} beams of a prompt need {K} cache rows at once: batch_rows = {batch_rows} < num_beams; "
                         f"use batch_rows >= {K}")
    if int(num_return_sequences) < 1 or int(num_return_sequences) > K:
        raise ValueError(f"{who}: num_return_sequences = {num_return_sequences}; 1 .. num_beams = {K} (a prompt keeps at most num_beams "
                         "finished hypotheses)")
    if list(additional_stop_symbols):
        raise ValueError(f"{who}: only the EOS id ends a hypothesis, additional_stop_symbols have no beam form: pass none and cut the "
                         "text afterwards, or use generate_many")
    if temperature > 0:
        raise ValueError(f"{who}: beam search is deterministic, temperature = {temperature} > 0 has no meaning here: use temperature=0, "
                         "or generate_many(n=...) for best-of-n sampling")
    if float(repetition_penalty) != 1.0:
        raise ValueError(f"{who}: beam scores are sums of raw log-probs, repetition_penalty = {repetition_penalty} has no beam form: use "
                         "repetition_penalty=1.0, or generate_many")
    if int(lookup or 0):
        raise ValueError(f"{who}: lookup decoding verifies drafts against ONE greedy continuation, beams have {K}: use lookup=0, or "
                         "generate_many(lookup=...)")
    return K


class BeamState:
    """The device state of G groups of K rows (include/a3vlm_hip.h, "Beam search"); every group starts done (empty)."""

    def __init__(self, G: int, K: int, ld_tok: int, device):
        R = G * K
        self.G, self.K, self.ld_tok = G, K, ld_tok
        z = lambda n, dt: torch.zeros(n, dtype=dt, device=device)
        self.cum = torch.full((R,), float("-inf"), dtype=torch.float32, device=device)
        self.alive = z(R, torch.uint8)
        self.state = torch.full((R,), -1, dtype=torch.int32, device=device)
        self.parent = torch.arange(R, dtype=torch.int32, device=device)
        self.next_tok = z(R, torch.int64)
        self.pos = torch.full((R,), -1, dtype=torch.int32, device=device)
        self.tail_lo = z(R, torch.int32)
        self.glen, self.base, self.limit = z(G, torch.int32), z(G, torch.int32), z(G, torch.int32)
        self.done = torch.ones(G, dtype=torch.uint8, device=device)
        self.pool_n, self.pool_added = z(G, torch.int32), z(G, torch.int32)
        self.pool_score, self.pool_cum = z((G, K), torch.float32), z((G, K), torch.float32)
        self.pool_len, self.pool_seq = z((G, K), torch.int32), z((G, K), torch.int32)
        self.pool_ids = z((G, K, ld_tok), torch.int64)
        self.tokens = [z((R, ld_tok), torch.int64), z((R, ld_tok), torch.int64)]       # read from [0], written to [1], swapped per step
        self.cand_score = z((G, 2 * K), torch.float32)
        self.cand_beam, self.cand_tok = z((G, 2 * K), torch.int32), z((G, 2 * K), torch.int32)
        self.lse = z(R, torch.float32)

    def start(self, g: int, base: int, limit: int, state0: int = -1) -> None:
        """A fresh prompt in group g: cum = [0, -inf, ...], only beam 0 alive, an empty pool."""
        K = self.K
        r = slice(g * K, g * K + K)
        self.cum[r] = float("-inf")
        self.cum[g * K] = 0.0
        self.alive[r] = 0
        self.alive[g * K] = 1
        self.state[r] = state0
        self.parent[r] = torch.arange(g * K, g * K + K, dtype=torch.int32, device=self.parent.device)
        self.next_tok[r] = 0
        self.pos[r] = -1
        self.tail_lo[r] = base
        self.glen[g], self.done[g], self.base[g], self.limit[g], self.pool_n[g], self.pool_added[g] = 0, 0, base, limit, 0, 0

    def step(self, logits: torch.Tensor, V: int, eos: int, early_stopping: bool, len_div: torch.Tensor, pos_cap: int, trans=None) -> None:
        """lse -> select -> advance on the raw logits [R, V]; swaps the token buffers."""
        ops.logits_prepare(logits, None, 1.0, None, self.lse)
        ops.beam_select(logits, self.lse, self.cum, self.alive, self.K, self.cand_score, self.cand_beam, self.cand_tok, trans=trans,
                        state=self.state if trans is not None else None)
        ops.beam_advance(self.cand_score, self.cand_beam, self.cand_tok, self, self.tokens[0], self.tokens[1], V, eos, early_stopping, len_div,
                         pos_cap, trans=trans)
        self.tokens.reverse()

    def harvest(self, g: int):
        """The group's pool, best first (score descending, then entry order): [(score, cum, ids)].  One host read."""
        n = int(self.pool_n[g].item())
        sc, cu = self.pool_score[g, :n].tolist(), self.pool_cum[g, :n].tolist()
        ln, sq, ids = self.pool_len[g, :n].tolist(), self.pool_seq[g, :n].tolist(), self.pool_ids[g, :n].tolist()
        order = sorted(range(n), key=lambda j: (-sc[j], sq[j]))
        return [(sc[j], cu[j], ids[j][:ln[j]]) for j in order]


@torch.no_grad()
def beam_search(model, prompts: List[str], images: Optional[torch.Tensor] = None, *, num_beams: int, batch_rows: int, max_gen_len=512,
                length_penalty: float = 1.0, early_stopping: bool = True, num_return_sequences: int = 1, constraint=None,
                return_ids: bool = False, return_scores: bool = False, poll_every: int = 4, additional_stop_symbols: Iterable[str] = (),
                temperature: float = 0.0, repetition_penalty: float = 1.0, lookup=None):
    """See ``MetaModel.beam_search``."""
    from .ragged import GroupScheduler
    if isinstance(prompts, str):
        raise ValueError(f"{model.__class__}.beam_search expects a LIST of prompts, but str is given")
    K = check_beam_args(num_beams, batch_rows, num_return_sequences, temperature=temperature, repetition_penalty=repetition_penalty,
                        additional_stop_symbols=additional_stop_symbols, lookup=lookup)
    nret = int(num_return_sequences)
    automaton = model.constraint_automaton(constraint)
    llma = model.llma
    llma._ragged_check("beam_search")                         # before anything is allocated or launched
    dev = model._device
    args = llma.args
    N, V, eos = len(prompts), args.vocab_size, model.tokenizer.eos_id
    G = int(batch_rows) // K
    R = G * K                                                 # rows beyond whole groups are not used
    assert 0 < R <= args.max_batch_size, (R, args.max_batch_size)
    mgl = [int(max_gen_len)] * N if isinstance(max_gen_len, int) else [int(x) for x in max_gen_len]
    assert len(mgl) == N, (len(mgl), N)
    if images is not None:
        images = images.to(dev)
        assert images.shape[0] == N, (tuple(images.shape), N)
    W = llma.image_words if images is not None else 0
    max_seq_len = args.max_seq_len - W
    prompt_tokens, limits = [], []
    for x, mg in zip(prompts, mgl):                           # truncation and limits per prompt: generate_many's
        t = model.tokenizer.encode(x, bos=True, eos=False)
        limits.append(min(max_seq_len, mg + len(t)))
        prompt_tokens.append(t[-(max_seq_len - mg):])
    lens = [len(t) for t in prompt_tokens]
    results: List[list] = [[] for _ in range(N)]
    model.last_beam_prefills = 0
    if N:
        max_new = max(max(lim - ln for lim, ln in zip(limits, lens)), 1)
        st = BeamState(G, K, max_new, dev)
        len_div = len_div_table(max_new + 2, length_penalty).to(dev)
        trans = automaton.device_table(dev) if automaton is not None else None
        state0 = automaton.start if automaton is not None else -1
        sched = GroupScheduler(lens, limits, R, W, K)
        llma.allocate_rows(R)
        smax = llma._k_cache[0].shape[2]
        logits = torch.zeros((R, V), dtype=torch.float32, device=dev)
        src_row = torch.arange(R, dtype=torch.int32, device=dev)
        shared = torch.zeros(R, dtype=torch.int32, device=dev)
        ptrs = None
        group_of = {}                                         # group -> prompt

        def release(g: int) -> None:
            results[group_of.pop(g)] = st.harvest(g)
            for r in range(g * K, g * K + K):
                sched.release(r)

        while True:
            for i, rows in sched.refill():
                lead = rows[0]
                assert lead % K == 0 and rows == list(range(lead, lead + K)), rows      # whole groups are released together
                g = lead // K
                t = torch.tensor(prompt_tokens[i], dtype=torch.long, device=dev)
                logits[lead].copy_(llma.prefill_row(lead, t[None], None if images is None else images[i:i + 1])[0])
                model.last_beam_prefills += 1
                src_row[lead:lead + K] = lead
                shared[lead] = 0
                if K > 1:                                     # the siblings start from the leader's logits and read its prefix
                    logits[lead + 1:lead + K] = logits[lead]
                    shared[lead + 1:lead + K] = llma.share_prefix(lead, src_row.new_tensor(rows[1:]), W + lens[i])
                st.start(g, W + lens[i], limits[i] - lens[i], state0)
                group_of[g] = i
            sched.finished_at_once.clear()                    # a prompt with nothing to write keeps its empty result
            if not sched.occupied():
                break
            st.step(logits, V, eos, early_stopping, len_div, smax, trans)
            pos_max = sched.advance()
            # generated[] counts this step's token: the tails hold one position less
            tail_max = max(sched.generated[g * K] for g in group_of) - 1
            if tail_max > 0 and K > 1:
                ptrs = ops.kv_permute_tails(llma._k_cache, llma._vt_cache, st.parent, st.tail_lo, st.pos, tail_max, K, ptrs)
            if sched.steps % poll_every == 0 or all(sched.generated[g * K] >= limits[i] - lens[i] for g, i in group_of.items()):
                done = st.done.tolist()
                for g in [g for g in group_of if done[g]]:
                    release(g)
                if not sched.occupied():
                    continue                                  # refill (or leave) before another step
            llma.forward_inference_rows(st.next_tok, st.pos, pos_max, out=logits, src_row=src_row, shared=shared)

    texts, ids, scores = [], [], []
    for hyps in results:
        hyps = hyps[:nret]
        t = [h[2] for h in hyps]
        s = [{"sum": h[1], "score": h[0]} for h in hyps]
        d = [model.tokenizer.decode(x) for x in t]
        if nret == 1:                                         # an empty pool (no hypothesis at all): the empty answer
            t, s, d = (t[0], s[0], d[0]) if hyps else ([], {"sum": float("-inf"), "score": float("-inf")}, "")
        texts.append(d)
        ids.append(t)
        scores.append(s)
    ret = (texts, ids) if return_ids else texts
    if return_scores:
        ret = ret + (scores,) if return_ids else (texts, scores)
    return ret
