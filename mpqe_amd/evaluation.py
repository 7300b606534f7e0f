"""Evaluation loop of the reference (utils.py:25-95): ROC-AUC with one sampled negative per
query and percentile rank of the target among all of a query's negatives, both through
`enc_dec.forward(formula, queries, targets, neg_nodes=flat, neg_lengths=lengths)` -- the ragged scoring form
whose `repeat_interleave` row map is mpqe_cosine_fwd's `q_row` (include/mpqe_amd.h).

Same call signatures, same python `random` stream for the sampled negatives (seeded per call, as the
reference does), same batch slicing. The two metrics are restated in numpy so nothing here needs sklearn or
scipy; tests/test_evaluation.py checks them against both.
"""
import random

import numpy as np


def roc_auc(labels, scores):
    """Area under the ROC curve = P(score of a positive > score of a negative) + 0.5 P(tie): the
    Mann-Whitney statistic on average ranks (what sklearn.metrics.roc_auc_score returns)."""
    labels = np.asarray(labels).astype(bool)
    scores = np.asarray(scores, dtype=np.float64)
    n_pos, n_neg = int(labels.sum()), int((~labels).sum())
    if n_pos == 0 or n_neg == 0:
        raise ValueError('Only one class present in y_true. ROC AUC score is not defined in that case.')
    order = np.argsort(scores, kind='mergesort')
    s = scores[order]
    ranks = np.empty(len(s), dtype=np.float64)
    i = 0
    while i < len(s):                       # average rank over each run of equal scores
        j = i
        while j + 1 < len(s) and s[j + 1] == s[i]:
            j += 1
        ranks[order[i:j + 1]] = 0.5 * (i + j) + 1.0
        i = j + 1
    return (ranks[labels].sum() - n_pos * (n_pos + 1) / 2.0) / (n_pos * n_neg)


def percentile_of_score(a, score):
    """scipy.stats.percentileofscore(a, score) with its default kind='rank'."""
    a = np.asarray(a, dtype=np.float64)
    n = len(a)
    if n == 0:
        return np.nan
    left, right = int((a < score).sum()), int((a <= score).sum())
    return (left + right + (1 if right > left else 0)) * 50.0 / n


def _get_perc_scores(scores, lengths):
    out, start = [], 0
    neg_scores = scores[len(lengths):]
    for i, length in enumerate(lengths):
        out.append(percentile_of_score(neg_scores[start:start + length], scores[i]))
        start += length
    return out


def _batches(formula_queries, batch_size):
    for offset in range(0, len(formula_queries), batch_size):
        yield offset, min(offset + batch_size, len(formula_queries))


def _on_device(test_queries):
    """How the dict's values hold the queries: 'sets' -- kg.QuerySets by formula --, 'mixed' -- kg.MixedQuerySets by query
    type (both the device route) -- or False for lists of Query. One kind per dict."""
    from .kg import MixedQuerySet, QuerySet
    kinds = {'mixed' if isinstance(v, MixedQuerySet) else 'sets' if isinstance(v, QuerySet) else 'lists'
             for v in test_queries.values()}
    if len(kinds) > 1:
        raise TypeError('evaluation: every formula\'s queries as a kg.QuerySet, every query type\'s as a kg.MixedQuerySet, '
                        'or every formula\'s as a list of Query')
    kind = kinds.pop() if kinds else 'lists'
    return False if kind == 'lists' else kind


def auc_batch_seed(seed, formula_position, batch_position):
    """The seed of the negatives' draw for one batch of eval_auc_queries over QuerySets: seed * 2^40 + formula position *
    2^20 + batch position (mod 2^64) -- the formula's position in the dict's iteration order, the batch's among the
    formula's windows [lo, lo + batch_size). Distinct for distinct (formula, batch), both below 2^20."""
    if not (0 <= formula_position < 2 ** 20 and 0 <= batch_position < 2 ** 20):
        raise ValueError('eval_auc_queries: at most 2^20 formulas and 2^20 batches a formula')
    return (int(seed) * 2 ** 40 + formula_position * 2 ** 20 + batch_position) & (2 ** 64 - 1)


def _eval_auc_sets(test_sets, enc_dec, batch_size, hard_negatives, seed, lib):
    """eval_auc_queries over {formula: kg.QuerySet}: ids and scores stay on the device. Per batch one draw of the library's
    sampler (sampling.NegativeSampler.from_csr over the set's own lists -- also for a 1-chain, as the reference's
    evaluation has it, unlike margin_loss) with auc_batch_seed's seed, one enc_dec.score_ids call; per formula the target
    and negative scores fill two buffers [Q] and one ops.eval_auc gives the integer statistic; one more over all formulas."""
    import torch

    from . import ops
    from .sampling import NegativeSampler
    formula_aucs, all_pos, all_neg, errs = {}, [], [], {}
    for f, (formula, qs) in enumerate(test_sets.items()):
        Q, dev = len(qs), qs.index.device
        if hard_negatives and qs.hard is None:
            raise Exception("Hard negative examples can only be used with "
                            "intersection queries")                   # reference model.py:467-469
        sampler = NegativeSampler.from_csr(qs.neg, qs.hard, dev, lib=lib)
        sampler.err = errs.setdefault(dev, sampler.err)         # one error word for all formulas: read once, below
        pos = torch.empty(Q, dtype=torch.float32, device=dev)
        neg = torch.empty(Q, dtype=torch.float32, device=dev)
        for b, (lo, hi) in enumerate(_batches(qs.targets, batch_size)):
            window = torch.arange(lo, hi, dtype=torch.long, device=dev)
            negatives = sampler.sample(window, auc_batch_seed(seed, f, b), hard_negatives)
            offsets = torch.arange(hi - lo + 1, dtype=torch.long, device=dev)
            scores = enc_dec.score_ids(formula, qs.anchors[lo:hi], qs.targets[lo:hi], neg=(negatives, offsets))
            pos[lo:hi] = scores[:hi - lo].to(dev)
            neg[lo:hi] = scores[hi - lo:].to(dev)
        formula_aucs[formula] = ops.auc_from_statistic(ops.eval_auc(pos, neg, lib=lib), Q, Q)
        all_pos.append(pos)
        all_neg.append(neg)
    for err in errs.values():
        ops.raise_on_flags(err)         # (an empty list: IndexError, the reference's random.choice([]))
    pos, neg = torch.cat(all_pos), torch.cat(all_neg)
    return ops.auc_from_statistic(ops.eval_auc(pos, neg, lib=lib), pos.shape[0], neg.shape[0]), formula_aucs


def _eval_perc_sets(test_sets, enc_dec, batch_size, hard_negatives, lib):
    """eval_perc_queries over {formula: kg.QuerySet}: per window the CSR of ALL its negatives is sliced with the offsets'
    host mirror (lengths only), enc_dec.score_ids scores targets and negatives, ops.eval_counts counts; the float64
    percentiles stay on the device and so does their mean -- one 8-byte read at the end."""
    import torch

    from . import ops
    percentiles, errs = [], {}
    for formula, qs in test_sets.items():
        dev = qs.index.device
        if hard_negatives and qs.hard is None:
            raise Exception("Hard negative examples can only be used with "
                            "intersection queries")
        pair, host = (qs.hard, qs.offsets_host(True)) if hard_negatives else (qs.neg, qs.offsets_host(False))
        if dev not in errs:
            errs[dev] = ops.new_error_word(dev)         # one error word for all windows: read once, below
        err = errs[dev]
        for lo, hi in _batches(qs.targets, batch_size):
            a, b = int(host[lo]), int(host[hi])
            offsets = pair[1][lo:hi + 1] - a
            scores = enc_dec.score_ids(formula, qs.anchors[lo:hi], qs.targets[lo:hi], neg=(pair[0][a:b], offsets))
            counts = ops.eval_counts(scores.to(dev), offsets, hi - lo, lib=lib, err=err)
            percentiles.append(ops.eval_percentiles(counts, offsets))
    if not percentiles:
        return np.mean([])
    mean = torch.cat(percentiles).mean()
    for err in errs.values():
        ops.raise_on_flags(err)
    return np.float64(mean.item())


def auc_window_seed(seed, type_position, window_position):
    """The seed of the negatives' draw for one window of eval_auc_queries over MixedQuerySets: seed * 2^40 + type position
    * 2^20 + window position (mod 2^64) -- the query type's position in the dict's iteration order, the window's among the
    type's windows [lo, lo + batch_size) over its concatenation. Distinct for distinct (type, window), both below 2^20.
    auc_batch_seed's form with the type in the formula's place: the windows differ from the QuerySet route's, and so do
    the draws."""
    if not (0 <= type_position < 2 ** 20 and 0 <= window_position < 2 ** 20):
        raise ValueError('eval_auc_queries: at most 2^20 query types and 2^20 windows a type')
    return (int(seed) * 2 ** 40 + type_position * 2 ** 20 + window_position) & (2 ** 64 - 1)


def _score_window(enc_dec, ms, lo, hi, neg, offsets_host):
    """the scores of queries [lo, hi) of a MixedQuerySet in forward()'s layout: one score_ids_mixed call over the type's
    formulas where the model has it, the window's runs of equal formula through score_ids otherwise"""
    if hasattr(enc_dec, 'score_ids_mixed'):
        return enc_dec.score_ids_mixed(ms.formulas, ms.formula_of[lo:hi], ms.anchors[lo:hi], ms.targets[lo:hi], neg=neg)
    from .model import score_ids_by_runs
    return score_ids_by_runs(enc_dec, ms.formulas, ms.formula_of_host[lo:hi], ms.anchors[lo:hi], ms.targets[lo:hi], neg,
                             offsets_host)


def _eval_auc_mixed(test_sets, enc_dec, batch_size, hard_negatives, seed, lib):
    """eval_auc_queries over {query type: kg.MixedQuerySet}. Per type ONE sampler over the concatenated lists; per window
    one draw (auc_window_seed) and one scoring call; per call one ops.eval_auc_segments over every formula of every type
    (one copy of [S] integers gives the {formula: AUC} dict) and one ops.eval_auc for the overall figure."""
    import torch

    from . import ops
    from .sampling import NegativeSampler
    all_pos, all_neg, errs, formulas, bounds, base = [], [], {}, [], [np.zeros(1, dtype=np.int64)], 0
    for t, (qt, ms) in enumerate(test_sets.items()):
        Q, dev = len(ms), ms.index.device
        if hard_negatives and ms.hard is None:
            raise Exception("Hard negative examples can only be used with "
                            "intersection queries")                   # reference model.py:467-469
        sampler = NegativeSampler.from_csr(ms.neg, ms.hard, dev, lib=lib)
        sampler.err = errs.setdefault(dev, sampler.err)         # one error word for all types: read once, below
        pos = torch.empty(Q, dtype=torch.float32, device=dev)
        neg = torch.empty(Q, dtype=torch.float32, device=dev)
        unit = np.arange(min(batch_size, Q) + 1, dtype=np.int64)
        for w, (lo, hi) in enumerate(_batches(ms.targets, batch_size)):
            window = torch.arange(lo, hi, dtype=torch.long, device=dev)
            negatives = sampler.sample(window, auc_window_seed(seed, t, w), hard_negatives)
            offsets = torch.arange(hi - lo + 1, dtype=torch.long, device=dev)
            scores = _score_window(enc_dec, ms, lo, hi, (negatives, offsets), unit[:hi - lo + 1])
            pos[lo:hi] = scores[:hi - lo].to(dev)
            neg[lo:hi] = scores[hi - lo:].to(dev)
        all_pos.append(pos)
        all_neg.append(neg)
        formulas += list(ms.formulas)
        bounds.append(ms.bounds[1:] + base)
        base += Q
    for err in errs.values():
        ops.raise_on_flags(err)         # (an empty list: IndexError, the reference's random.choice([]))
    pos, neg = torch.cat(all_pos), torch.cat(all_neg)
    bounds = np.concatenate(bounds)
    sizes = np.diff(bounds)
    if (sizes == 0).any():
        raise ValueError('Only one class present in y_true. ROC AUC score is not defined in that case.')
    off = torch.from_numpy(bounds).to(pos.device)
    u2 = ops.eval_auc_segments(pos, neg, off, off, lib=lib).cpu().tolist()
    formula_aucs = {f: ops.auc_from_statistic(u & (2 ** 64 - 1), int(n), int(n)) for f, u, n in zip(formulas, u2, sizes)}
    return ops.auc_from_statistic(ops.eval_auc(pos, neg, lib=lib), pos.shape[0], neg.shape[0]), formula_aucs


def _eval_perc_mixed(test_sets, enc_dec, batch_size, hard_negatives, lib):
    """eval_perc_queries over {query type: kg.MixedQuerySet}: _eval_perc_sets' windows over a type's concatenation"""
    import torch

    from . import ops
    percentiles, errs = [], {}
    for qt, ms in test_sets.items():
        dev = ms.index.device
        if hard_negatives and ms.hard is None:
            raise Exception("Hard negative examples can only be used with "
                            "intersection queries")
        pair, host = (ms.hard, ms.offsets_host(True)) if hard_negatives else (ms.neg, ms.offsets_host(False))
        if dev not in errs:
            errs[dev] = ops.new_error_word(dev)         # one error word for all windows: read once, below
        err = errs[dev]
        for lo, hi in _batches(ms.targets, batch_size):
            a, b = int(host[lo]), int(host[hi])
            offsets = pair[1][lo:hi + 1] - a
            scores = _score_window(enc_dec, ms, lo, hi, (pair[0][a:b], offsets), host[lo:hi + 1] - a)
            counts = ops.eval_counts(scores.to(dev), offsets, hi - lo, lib=lib, err=err)
            percentiles.append(ops.eval_percentiles(counts, offsets))
    if not percentiles:
        return np.mean([])
    mean = torch.cat(percentiles).mean()
    for err in errs.values():
        ops.raise_on_flags(err)
    return np.float64(mean.item())


def eval_auc_queries(test_queries, enc_dec, batch_size=128, hard_negatives=False, seed=0, lib=None):
    """-> (overall AUC, {formula: AUC}). One negative per query, drawn with random.choice after
    random.seed(seed) (reference utils.py:34-69).

    {formula: kg.QuerySet} (KGIndex.sample_query_sets) takes the device route: same windows [lo, lo + batch_size), same
    metric -- ops.eval_auc's integer Mann-Whitney statistic, which is roc_auc(np.nan_to_num(scores)) to the bit -- with no id
    list and no score on the host; enc_dec scores through score_ids(formula, anchors, targets, neg). The one negative per
    query comes from the library's counter stream (mpqe_sample_negatives, seeded per batch by auc_batch_seed), NOT from
    Python's Mersenne Twister: for a given `seed` the draws differ from the list path's -- the same distribution, other
    numbers; the deviation sampling.py states. lib: the stand-in library of the sets' index (kg.KGIndex(lib=...)), if any.

    {query type: kg.MixedQuerySet} (MixedQuerySet.from_sets) is the device route over queries of DIFFERENT formulas at once:
    the windows are [lo, lo + batch_size) over a type's concatenation, each one sampler draw (auc_window_seed's seed: for a
    given `seed` other negatives than the QuerySet route's -- the same deviation) and one scoring call --
    enc_dec.score_ids_mixed where the model has it (QueryEncoderDecoder: ONE launch; RGCNEncoderDecoder: two, whatever the
    number of formulas; either walks the runs itself where its launch does not cover the model), the runs of a window
    through score_ids otherwise; the
    {formula: AUC} dict comes from ONE ops.eval_auc_segments and one copy of its integers."""
    kind = _on_device(test_queries)
    if kind == 'mixed':
        return _eval_auc_mixed(test_queries, enc_dec, batch_size, hard_negatives, seed, lib)
    if kind:
        return _eval_auc_sets(test_queries, enc_dec, batch_size, hard_negatives, seed, lib)
    predictions, labels, formula_aucs = [], [], {}
    random.seed(seed)
    for formula in test_queries:
        formula_labels, formula_predictions = [], []
        formula_queries = test_queries[formula]
        for lo, hi in _batches(formula_queries, batch_size):
            batch_queries = formula_queries[lo:hi]
            pool = 'hard_neg_samples' if hard_negatives else 'neg_samples'
            negatives = [random.choice(getattr(formula_queries[j], pool)) for j in range(lo, hi)]
            lengths = [1] * (hi - lo)
            formula_labels.extend([1] * len(lengths) + [0] * len(negatives))
            targets = [q.target_node for q in batch_queries]
            scores = enc_dec.forward(formula, batch_queries, targets, neg_nodes=negatives, neg_lengths=lengths)
            formula_predictions.extend(scores.detach().cpu().tolist())
        formula_aucs[formula] = roc_auc(formula_labels, np.nan_to_num(formula_predictions))
        labels.extend(formula_labels)
        predictions.extend(formula_predictions)
    return roc_auc(labels, np.nan_to_num(predictions)), formula_aucs


def eval_perc_queries(test_queries, enc_dec, batch_size=128, hard_negatives=False, lib=None):
    """-> mean percentile rank of the target's score among ALL negatives of its query (reference utils.py:72-95).

    {formula: kg.QuerySet} takes the device route (see eval_auc_queries): ops.eval_counts per window, the per-query
    percentiles -- percentile_of_score's to the bit -- and their mean in float64 on the device. The mean may differ from
    np.mean's by the order of the additions: at most Q * 2^-52 relative over Q non-negative terms.
    {query type: kg.MixedQuerySet}: the same per-query percentiles from windows over a type's concatenation, one scoring
    call and one ops.eval_counts a window (see eval_auc_queries)."""
    kind = _on_device(test_queries)
    if kind == 'mixed':
        return _eval_perc_mixed(test_queries, enc_dec, batch_size, hard_negatives, lib)
    if kind:
        return _eval_perc_sets(test_queries, enc_dec, batch_size, hard_negatives, lib)
    perc_scores = []
    for formula in test_queries:
        formula_queries = test_queries[formula]
        for lo, hi in _batches(formula_queries, batch_size):
            batch_queries = formula_queries[lo:hi]
            pool = 'hard_neg_samples' if hard_negatives else 'neg_samples'
            lengths = [len(getattr(formula_queries[j], pool)) for j in range(lo, hi)]
            negatives = [n for j in range(lo, hi) for n in getattr(formula_queries[j], pool)]
            targets = [q.target_node for q in batch_queries]
            scores = enc_dec.forward(formula, batch_queries, targets, neg_nodes=negatives, neg_lengths=lengths)
            perc_scores.extend(_get_perc_scores(scores.detach().cpu().tolist(), lengths))
    return np.mean(perc_scores)


def _rank_sets(test_sets, enc_dec, batch_size, index):
    """eval_rank_queries over {formula: kg.QuerySet}: per window the answers on the device (index.answers over the anchor
    ids) and one enc_dec.rank_ids call; the ranks stay on the device and are copied once per set. Yields (formula, ranks)."""
    import torch
    for formula, qs in test_sets.items():
        parts = []
        for lo, hi in _batches(qs.targets, batch_size):
            exclude = None if index is None else index.answers(formula, qs.anchors[lo:hi])
            parts.append(enc_dec.rank_ids(formula, qs.anchors[lo:hi], qs.targets[lo:hi], exclude)[0])
        yield formula, (torch.cat(parts).cpu().numpy() if parts else np.zeros(0, dtype=np.int64))


def _rank_mixed_sets(test_sets, enc_dec, batch_size, index):
    """eval_rank_queries over {query type: kg.MixedQuerySet}: per window of a type's concatenation the records from the
    device ids (index.records_of_ids), the answers of queries of different formulas in one launch (index.answers_mixed)
    and ONE ranking call -- enc_dec.rank_ids_mixed where the model has it, the window's runs through rank_ids otherwise;
    the ranks stay on the device and are copied once per type. Yields (formula, ranks) from the type's bounds."""
    import torch
    for qt, ms in test_sets.items():
        parts = []
        for lo, hi in _batches(ms.targets, batch_size):
            fo, anchors, targets = ms.formula_of[lo:hi], ms.anchors[lo:hi], ms.targets[lo:hi]
            exclude = None
            if index is not None:
                exclude = index.answers_mixed(qt, index.records_of_ids(ms.formulas, fo, anchors, targets))
            if hasattr(enc_dec, 'rank_ids_mixed'):
                ranks = enc_dec.rank_ids_mixed(ms.formulas, fo, anchors, targets, exclude)[0]
            else:
                from .model import rank_ids_by_runs
                ranks = rank_ids_by_runs(enc_dec, ms.formulas, ms.formula_of_host[lo:hi], anchors, targets, exclude)[0]
            parts.append(ranks)
        ranks = torch.cat(parts).cpu().numpy() if parts else np.zeros(0, dtype=np.int64)
        for f, formula in enumerate(ms.formulas):
            yield formula, ranks[int(ms.bounds[f]):int(ms.bounds[f + 1])]


def eval_rank_queries(test_queries, enc_dec, batch_size=128, ks=(1, 3, 10), known_answers=None):
    """Link-prediction metrics over ALL entities of each query's target mode (no counterpart in the reference, whose
    evaluation ranks the target among the negatives stored with the query): the rank of query.target_node from
    `enc_dec.rank_targets`, filtered by `known_answers[query]` (every entity known to answer the query; the target is
    never filtered out) when given -- the standard filtered setting -- raw otherwise. known_answers may also be a
    kg.KGIndex: the answers of each batch are then computed on the device (index.answers) and never visit the host.
    -> {'mrr', 'hits@k' for k in ks, 'num_queries', 'per_formula': {formula: {'mrr', 'hits@k', 'num_queries'}}}.

    {formula: kg.QuerySet} and {query type: kg.MixedQuerySet} take the device route (known_answers: a kg.KGIndex or
    None): windows [lo, lo + batch_size), the answers from index.answers / index.answers_mixed over the device ids, one
    enc_dec.rank_ids / rank_ids_mixed call a window -- for a MixedQuerySet one ranking call over queries of DIFFERENT
    formulas and target modes --, the ranks copied to the host once per set or type. The same ranks as the list route
    over QuerySet.queries(), so the same dict."""
    def summary(ranks):
        r = np.asarray(ranks, dtype=np.float64)
        out = {'mrr': float(np.mean(1.0 / r)) if r.size else float('nan')}
        for k in ks:
            out['hits@%d' % k] = float(np.mean(r <= k)) if r.size else float('nan')
        out['num_queries'] = int(r.size)
        return out

    from .kg import KGIndex
    kind = _on_device(test_queries)
    if kind:
        if known_answers is not None and not isinstance(known_answers, KGIndex):
            raise TypeError('eval_rank_queries: device query sets take known_answers as a kg.KGIndex (or None)')
        ranks_of = _rank_mixed_sets if kind == 'mixed' else _rank_sets
        all_ranks, per_formula = [], {}
        for formula, ranks in ranks_of(test_queries, enc_dec, batch_size, known_answers):
            per_formula[formula] = summary(ranks)
            all_ranks.append(ranks)
        out = summary(np.concatenate(all_ranks) if all_ranks else [])
        out['per_formula'] = per_formula
        return out
    all_ranks, per_formula = [], {}
    for formula in test_queries:
        formula_queries = test_queries[formula]
        formula_ranks = []
        for lo, hi in _batches(formula_queries, batch_size):
            batch_queries = formula_queries[lo:hi]
            if isinstance(known_answers, KGIndex):
                exclude = known_answers.answers(formula, batch_queries)
            else:
                exclude = None if known_answers is None else [list(known_answers[q]) for q in batch_queries]
            targets = [q.target_node for q in batch_queries]
            ranks = enc_dec.rank_targets(formula, batch_queries, targets, exclude=exclude)
            formula_ranks.extend(int(r) for r in ranks.detach().cpu().tolist())
        per_formula[formula] = summary(formula_ranks)
        all_ranks.extend(formula_ranks)
    out = summary(all_ranks)
    out['per_formula'] = per_formula
    return out
