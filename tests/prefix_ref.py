"""Pure restatement of prefix sharing in ``generate_many(prefix_sharing=True)``: how the prompt list is cut into runs, the shared
length P of a run, the order in which prompts are admitted to cache rows, and the held-row rule.  No torch, no project imports:
``a3vlm_amd.model.ragged.prefix_groups`` / ``PrefixScheduler`` must agree with it on every script (tests/test_prefix_cpu.py).

A prompt's cache is [BOS | W image words | text].  A run = adjacent prompts with equal image key whose P stays > 0, grown greedily:
  C = W + (longest common token prefix, BOS included);  P = min(C, W + shortest member - 1) rounded DOWN to 64;
  P counts as 0 when an image is present and P < W + 1 (the prefix is prefilled with the whole image in front).
``round_p=False`` / ``hold=False`` are the two mutants the tests must catch."""


def lcp(a, b):
    n = 0
    while n < len(a) and n < len(b) and a[n] == b[n]:
        n += 1
    return n


def run_p(toks, W, round_p=True):
    common = min(lcp(toks[0], t) for t in toks)
    P = min(W + common, W + min(len(t) for t in toks) - 1)
    if round_p:
        P -= P % 64
    return P if P > 0 and (W == 0 or P >= W + 1) else 0


def runs(tokens, keys, W, round_p=True):
    out, i = [], 0
    while i < len(tokens):
        j, P = i + 1, 0
        while j < len(tokens) and keys[j] == keys[i] and run_p(tokens[i:j + 1], W, round_p) > 0:
            P = run_p(tokens[i:j + 1], W, round_p)
            j += 1
        out.append((list(range(i, j)), P if j - i > 1 else 0))
        i = j
    return out


def simulate(lens, limits, R, groups, finish_order, hold=True):
    """Event script: admit as far as possible, then the prompt ``finish_order[k]`` finishes, admit again, ...  Returns the list of
    admissions (prompt, row, leader row or None, prefix prefilled now?) in the order they happen.  A prompt that is not running
    when its turn to finish comes is an error of the script."""
    run_of = {i: g for g, (ms, _) in enumerate(groups) for i in ms}
    row_of, leader, left, log = {}, {}, {}, []
    nxt = 0

    def admit():
        nonlocal nxt
        while nxt < len(lens):
            g = run_of[nxt]
            ms, P = groups[g]
            if limits[nxt] <= lens[nxt]:
                if P and nxt == ms[0]:
                    left[g] = len(ms)
                if P:
                    left[g] -= 1
                nxt += 1
                continue
            busy = set(row_of.values())
            kept = {leader[h] for h in leader if left.get(h, 0) > 0 and h != g} if hold else set()
            free = [r for r in range(R) if r not in busy and r not in kept]
            if not free:
                return
            if P and nxt == ms[0]:
                left[g] = len(ms)
            r = free[0]
            new = bool(P) and (g not in leader or left[g] == len(ms) and nxt == ms[0])
            if P and g not in leader:
                leader[g] = r
            row_of[nxt] = r
            log.append((nxt, r, leader[g] if P else None, new if P else None))
            nxt += 1

    admit()
    for i in finish_order:
        del row_of[i]
        g = run_of[i]
        if groups[g][1]:
            left[g] -= 1
        admit()
    assert nxt == len(lens) and not row_of, "the script ends with every prompt finished"
    return log
