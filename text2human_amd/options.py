"""YAML option surface of the sampling path.

Mirrors the contract of the reference's utils/options.py:33-129 (same keys in,
same derived keys out) so `configs/sample_from_parsing.yml` /
`sample_from_pose.yml` parse unchanged:

* ``parse(path, is_train=False)`` -> ordered dict, plus ``is_train`` and
  ``opt['path'][root|results_root|log|visualization]`` (utils/options.py:56-79)
* ``dict_to_nonedict`` -> missing keys read as ``None`` (utils/options.py:105-129)
* ``gpu_ids`` is only echoed unless ``set_CUDA_VISIBLE_DEVICES`` is truthy
  (utils/options.py:47-52); on ROCm the variable that matters is
  ``HIP_VISIBLE_DEVICES`` and it is set alongside.
"""
import os
import os.path as osp
from collections import OrderedDict

import yaml


class NoneDict(dict):
    """dict whose missing keys read as None."""

    def __missing__(self, key):
        return None


def dict_to_nonedict(opt):
    if isinstance(opt, dict):
        return NoneDict((k, dict_to_nonedict(v)) for k, v in opt.items())
    if isinstance(opt, list):
        return [dict_to_nonedict(v) for v in opt]
    return opt


def _ordered_load(stream):

    class _Loader(yaml.SafeLoader):
        pass

    def _construct(loader, node):
        loader.flatten_mapping(node)
        return OrderedDict(loader.construct_pairs(node))

    _Loader.add_constructor(yaml.resolver.BaseResolver.DEFAULT_MAPPING_TAG,
                            _construct)
    return yaml.load(stream, Loader=_Loader)


def parse(opt_path, is_train=False, root=None):
    with open(opt_path, 'r') as f:
        opt = _ordered_load(f)

    gpu_list = ','.join(str(x) for x in opt.get('gpu_ids', []) or [])
    if opt.get('set_CUDA_VISIBLE_DEVICES', None):
        os.environ['CUDA_VISIBLE_DEVICES'] = gpu_list
        os.environ['HIP_VISIBLE_DEVICES'] = gpu_list
        print('export CUDA_VISIBLE_DEVICES=' + gpu_list, flush=True)
    else:
        print('gpu_list: ', gpu_list, flush=True)

    opt['is_train'] = is_train
    root = root or osp.abspath(os.getcwd())
    paths = OrderedDict(root=root)
    if is_train:
        raise NotImplementedError(
            'text2human_amd implements the sampling path only '
            '(training is out of scope, see DESIGN.md)')
    results_root = osp.join(root, 'results', opt['name'])
    paths['results_root'] = results_root
    paths['log'] = results_root
    paths['visualization'] = osp.join(results_root, 'visualization')
    opt['path'] = paths
    return opt


# Sampling order of the index sampler ("Confidence-ordered decoding").  Absent keys = the reference's loop.
SAMPLE_ORDERS = ('random', 'confidence')
CONFIDENCE_ROUNDS, CONFIDENCE_CHOICE_TEMP = 16, 4.5


def sampling_order(opt):
    """-> None for the reference's random-order loop (no `sample_order` key, or `random`), else
    (rounds, choice_temp) of `sample_order: confidence` with `confidence_rounds` / `confidence_choice_temp`
    (defaults 16 / 4.5).  Raises ValueError on an unknown order or values out of range."""
    order = opt.get('sample_order')
    if order is None or order == 'random':
        return None
    if order not in SAMPLE_ORDERS:
        raise ValueError(f'sample_order must be one of {SAMPLE_ORDERS}, got {order!r}')
    rounds, ct = opt.get('confidence_rounds'), opt.get('confidence_choice_temp')
    rounds = CONFIDENCE_ROUNDS if rounds is None else int(rounds)
    ct = CONFIDENCE_CHOICE_TEMP if ct is None else float(ct)
    if rounds < 1 or not ct >= 0.0:
        raise ValueError(f'confidence_rounds >= 1 and confidence_choice_temp >= 0 expected, got {rounds}, {ct}')
    return rounds, ct


# Truncated sampling ("Truncated sampling").  Absent keys = off = the reference's draw.
TOP_P_ONE = 1 << 20  # top_p travels as rint(top_p * 2^20) (include/t2h_hip.h, t2h_truncation_threshold)


def truncation_settings(top_k=None, top_p=None, n_class=None):
    """(top_k, top_p) of the public surface -> the validated (top_k, top_p_q) pair of the C structs; (0, 0) = off.
    top_k in {None, 0} or >= n_class is off, top_p in {None, 1.0} is off; valid are integers top_k >= 1 and
    0 < top_p <= 1 (ValueError naming the value otherwise -- callers check before the generator moves)."""
    import numbers
    k = 0
    if top_k is not None:
        if isinstance(top_k, bool) or not isinstance(top_k, numbers.Integral) or int(top_k) < 0:
            raise ValueError(f'top_k must be an integer >= 1 (None or 0: off), got {top_k!r}')
        k = min(int(top_k), 0x7fffffff)
        if n_class is not None and k >= int(n_class):
            k = 0
    p_q = 0
    if top_p is not None:
        if isinstance(top_p, bool) or not isinstance(top_p, numbers.Real):
            raise ValueError(f'top_p must be a number in (0, 1] (None or 1.0: off), got {top_p!r}')
        p = float(top_p)
        if not 0.0 < p <= 1.0:
            raise ValueError(f'top_p must lie in (0, 1] (None or 1.0: off), got {top_p!r}')
        p_q = int(round(p * TOP_P_ONE))  # (round half to even, like rint)
        if p_q == 0:
            raise ValueError(f'top_p is too small (it is resolved in steps of 2^-20), got {top_p!r}')
        if p_q == TOP_P_ONE:
            p_q = 0
    return k, p_q


def per_image_values(batch, value, what):
    """A sampling control given PER IMAGE ("Per-image sampling controls") -> the list of its `batch` entries
    as plain Python values, in the caller's sample order; None if `value` is what it always could be (a scalar or
    None).  Per image = a list, a tuple, a 1-D numpy array or a 1-D CPU tensor; a wrong length is a ValueError."""
    if isinstance(value, (list, tuple)):
        vals = list(value)
    elif getattr(value, 'ndim', 0) >= 1 and hasattr(value, 'tolist'):
        if value.ndim != 1:
            raise ValueError(f'{what}: one entry per image expected (a 1-D sequence), got shape {tuple(value.shape)}')
        vals = list(value.tolist())
    else:
        return None
    if len(vals) != int(batch):
        raise ValueError(f'{what}: one entry per image expected, got {len(vals)} entries for a batch of {int(batch)}')
    return vals


def is_per_image(value):
    """True iff `value` is a per-image sequence (per_image_values), whatever its length"""
    return isinstance(value, (list, tuple)) or (getattr(value, 'ndim', 0) >= 1 and hasattr(value, 'tolist'))


def sampling_truncation(opt):
    """-> (top_k, top_p) of the options `sample_top_k` / `sample_top_p` (None where absent), validated."""
    top_k, top_p = opt.get('sample_top_k'), opt.get('sample_top_p')
    truncation_settings(top_k, top_p)
    return top_k, top_p


# Best-of-N selection by per-token log-probability.  Absent key, or 1 = off = one plain call.
def best_of_value(n):
    """the validated candidate count of sample_best_of: an integer >= 1 (ValueError naming the value otherwise --
    callers check before anything is drawn)"""
    import numbers
    if isinstance(n, bool) or not isinstance(n, numbers.Integral) or int(n) < 1:
        raise ValueError(f'sample_best_of must be an integer >= 1 (1: off), got {n!r}')
    return int(n)


def sampling_best_of(opt):
    """-> the candidate count of the option `sample_best_of` (1 where absent: the existing path), validated."""
    n = opt.get('sample_best_of')
    return 1 if n is None else best_of_value(n)


# Sampled bottom-index refinement.  Absent keys = off = the argmax of the index-prediction heads.
REFINE_KEYS = ('refine_temp', 'refine_top_k', 'refine_top_p')


def refine_values(temp=None, top_k=None, top_p=None, batch=None):
    """The public refine_temp / refine_top_k / refine_top_p, validated: each a scalar or a per-image sequence
    (per_image_values; its length is checked against `batch` if given).  -> None if all three are None (sampling off),
    else (temp, top_k, top_p) with temp defaulting to 1.0.  ValueError names the option (and the image)."""
    import numbers
    if temp is None and top_k is None and top_p is None:
        return None
    temp = 1.0 if temp is None else temp
    for name, value in zip(REFINE_KEYS, (temp, top_k, top_p)):
        if batch is not None:
            vals = per_image_values(batch, value, name)
        else:
            vals = per_image_values(len(value) if isinstance(value, (list, tuple)) else value.shape[0], value,
                                    name) if is_per_image(value) else None
        for i, v in enumerate([value] if vals is None else vals):
            who = name if vals is None else f'{name}, image {i}'
            try:
                if name == 'refine_temp':
                    if isinstance(v, bool) or not isinstance(v, numbers.Real) or not float(v) > 0.0 or float(v) == float('inf'):
                        raise ValueError(f'must be a finite number > 0, got {v!r}')
                elif name == 'refine_top_k':
                    truncation_settings(v, None)
                else:
                    truncation_settings(None, v)
            except ValueError as e:
                raise ValueError(f'{who}: {e}') from None
    return temp, top_k, top_p


def refine_sampling(opt):
    """-> refine_values of the options `refine_temp` / `refine_top_k` / `refine_top_p` (None: absent, sampling off).
    The options are scalars, like `sample_top_k` / `sample_top_p`: a dataset run has no per-image identity."""
    vals = [opt.get(k) for k in REFINE_KEYS]
    for k, v in zip(REFINE_KEYS, vals):
        if is_per_image(v):
            raise ValueError(f'{k}: the option is one value for the whole run, got {v!r}')
    return refine_values(*vals)


# Per-image seeds.  Absent key = off = the shared generator stream of the reference.
def image_seeds(batch, seeds):
    """The validated `seeds` of a seeded sampling call: one integer in [0, 2^64) per image, in the caller's sample order
    (a list, a tuple, a 1-D numpy array or a 1-D CPU tensor of integers) -> list of `batch` Python ints.  ValueError
    naming the image otherwise -- callers check before anything is drawn or launched."""
    import numbers
    vals = per_image_values(batch, seeds, 'seeds')
    if vals is None:
        raise ValueError(f'seeds: one integer per image expected (a sequence of {int(batch)}), got {seeds!r}')
    for b, s in enumerate(vals):
        if isinstance(s, bool) or not isinstance(s, numbers.Integral):
            raise ValueError(f'seeds, image {b}: an integer expected, got {s!r}')
        if not 0 <= int(s) < (1 << 64):
            raise ValueError(f'seeds, image {b}: must lie in [0, 2^64), got {s!r}')
    return [int(s) for s in vals]


def image_seed(manual_seed, img_name):
    """The seed of one image of a `per_image_seeds` run: the first 8 bytes, big-endian, of
    SHA-256(f"{manual_seed}:{img_name}") -- a function of the run's seed and the image's name only, not of the dataset
    order, the batch size, the shard or the rank."""
    import hashlib
    return int.from_bytes(hashlib.sha256(f'{manual_seed}:{img_name}'.encode()).digest()[:8], 'big')


def per_image_seeding(opt):
    """-> True iff the option `per_image_seeds` is set (validated: a bool, or absent).  The flag promises that an image
    does not depend on its batch; the paths that cannot keep that promise yet -- `sample_order: confidence`,
    `sample_best_of` > 1, any `refine_*` key (those draws come from the shared generator) -- raise ValueError with it."""
    flag = opt.get('per_image_seeds')
    if flag is None or flag is False:
        return False
    if flag is not True:
        raise ValueError(f'per_image_seeds must be true or false, got {flag!r}')
    clash = []
    if sampling_order(opt) is not None:
        clash.append('sample_order: confidence')
    if sampling_best_of(opt) > 1:
        clash.append('sample_best_of > 1')
    clash += [k for k in REFINE_KEYS if opt.get(k) is not None]
    if clash:
        raise ValueError('per_image_seeds promises images that do not depend on their batch; it cannot be combined with '
                         + ', '.join(clash) + ' (those draws use the shared generator stream)')
    return True


# Self-correction.  `revise_passes` absent or 0 = off = today's run.
REVISE_FOLDS = (2, 4, 8, 16)
REVISE_ACCEPT = ('improve', 'always')
REVISE_FRACTION, REVISE_FOLDS_DEFAULT = 0.25, 4
PLL_BATCH_MAX = 32  # the critic's K evaluations run as ONE batch of K * B images while K * B <= this


def pll_batched(batch, folds):
    """True: the K evaluations of the pseudo-likelihood critic run as one batch of K * B images; False: as K calls at
    batch B.  A function of (B, K) alone."""
    return int(batch) * int(folds) <= PLL_BATCH_MAX


def revise_folds_value(folds):
    """the validated fold count of pll_fn / revise_fn (ValueError otherwise)"""
    if isinstance(folds, bool) or folds not in REVISE_FOLDS:
        raise ValueError(f'folds must be one of {REVISE_FOLDS}, got {folds!r}')
    return int(folds)


def revise_passes_value(passes, allow_zero=False):
    import numbers
    if isinstance(passes, bool) or not isinstance(passes, numbers.Integral) or int(passes) < (0 if allow_zero else 1):
        raise ValueError(f'revise passes must be an integer >= {0 if allow_zero else 1}, got {passes!r}')
    return int(passes)


def revise_fractions(batch, fraction):
    """fraction of revise_fn: a number in (0, 1], or one per image -> list of `batch` floats (ValueError otherwise)"""
    import numbers
    vals = per_image_values(batch, fraction, 'fraction')
    out = []
    for b, f in enumerate([fraction] * int(batch) if vals is None else vals):
        if isinstance(f, bool) or not isinstance(f, numbers.Real) or not 0.0 < float(f) <= 1.0:
            raise ValueError(f'fraction{"" if vals is None else f", image {b}"}: must lie in (0, 1], got {f!r}')
        out.append(float(f))
    return out


def revise_counts(batch, count):
    """count of revise_fn: an integer >= 0, or one per image -> list of `batch` ints (ValueError otherwise)"""
    import numbers
    vals = per_image_values(batch, count, 'count')
    out = []
    for b, c in enumerate([count] * int(batch) if vals is None else vals):
        if isinstance(c, bool) or not isinstance(c, numbers.Integral) or not 0 <= int(c) <= 0x7fffffff:
            raise ValueError(f'count{"" if vals is None else f", image {b}"}: must be an integer >= 0, got {c!r}')
        out.append(int(c))
    return out


def revise_row_counts(eligible, fraction=None, count=None):
    """Rows revise_fn redoes per image and pass: eligible = the rows of every image the caller does not keep.  With count
    min(count, eligible_b); otherwise max(1, floor(fraction * eligible_b + 0.5)) in float64, 0 where eligible_b = 0.
    Exactly one of fraction / count (validated here: ValueError)."""
    import math
    if (fraction is None) == (count is None):
        raise ValueError('revise: give either fraction or count, not both')
    batch = len(eligible)
    if count is not None:
        return [min(c, int(e)) for c, e in zip(revise_counts(batch, count), eligible)]
    return [0 if int(e) == 0 else max(1, int(math.floor(f * float(int(e)) + 0.5)))
            for f, e in zip(revise_fractions(batch, fraction), eligible)]


def revise_accept_value(accept):
    if accept not in REVISE_ACCEPT:
        raise ValueError(f'accept must be one of {REVISE_ACCEPT}, got {accept!r}')
    return accept


def revise_settings(opt):
    """-> None (no `revise_passes` key, or 0: off) or (passes, fraction, folds) of the options `revise_passes` /
    `revise_fraction` (default 0.25) / `revise_folds` (default 4), validated.  The options are scalars, one value for
    the whole run; all three are validated whether the feature is on or not.  `opt` is not changed."""
    passes = opt.get('revise_passes')
    passes = 0 if passes is None else revise_passes_value(passes, allow_zero=True)
    fraction, folds = opt.get('revise_fraction'), opt.get('revise_folds')
    if is_per_image(fraction):
        raise ValueError(f'revise_fraction: the option is one value for the whole run, got {fraction!r}')
    fraction = revise_fractions(1, REVISE_FRACTION if fraction is None else fraction)[0]
    folds = revise_folds_value(REVISE_FOLDS_DEFAULT if folds is None else folds)
    return (passes, fraction, folds) if passes > 0 else None


# Garment colour control.  No `recolor_upper` / `recolor_lower` / `recolor_outer` key = off = today's run.
RECOLOR_NAMES = ('upper', 'lower', 'outer')
RECOLOR_FEATHER_DEFAULT, RECOLOR_FEATHER_MAX, RECOLOR_LUMA_DEFAULT = 2, 8, 1.0


def recolor_colour(value, name='colour'):
    """an (r, g, b) colour of the recolouring: three numbers in [0, 1] -> tuple of floats (ValueError otherwise)"""
    import math
    import numbers
    if isinstance(value, (str, bytes)) or not hasattr(value, '__len__') or len(value) != 3:
        raise ValueError(f'{name}: a colour is three numbers r, g, b in [0, 1], got {value!r}')
    out = []
    for v in value:
        if isinstance(v, bool) or not isinstance(v, numbers.Real) or math.isnan(float(v)) or not 0.0 <= float(v) <= 1.0:
            raise ValueError(f'{name}: a colour is three numbers r, g, b in [0, 1], got {value!r}')
        out.append(float(v))
    return tuple(out)


def recolor_feather_value(feather):
    import numbers
    if isinstance(feather, bool) or not isinstance(feather, numbers.Integral) or not 0 <= int(feather) <= RECOLOR_FEATHER_MAX:
        raise ValueError(f'recolor_feather: must be an integer number of pixels in [0, {RECOLOR_FEATHER_MAX}], got {feather!r}')
    return int(feather)


def recolor_luma_value(luma):
    import math
    import numbers
    if isinstance(luma, bool) or not isinstance(luma, numbers.Real) or math.isnan(float(luma)) or not 0.0 <= float(luma) <= 1.0:
        raise ValueError(f'recolor_luma: must lie in [0, 1], got {luma!r}')
    return float(luma)


def recolor_settings(opt):
    """-> None (none of `recolor_upper` / `recolor_lower` / `recolor_outer` set: off) or (colours, feather, luma):
    colours = {'upper': (r, g, b), ...} of the keys that are set, `recolor_feather` (default 2) and `recolor_luma`
    (default 1.0), validated.  All five keys are validated whether the feature is on or not.  `opt` is not changed."""
    colours = {}
    for name in RECOLOR_NAMES:
        v = opt.get(f'recolor_{name}')
        if v is not None:
            colours[name] = recolor_colour(v, f'recolor_{name}')
    feather, luma = opt.get('recolor_feather'), opt.get('recolor_luma')
    feather = recolor_feather_value(RECOLOR_FEATHER_DEFAULT if feather is None else feather)
    luma = recolor_luma_value(RECOLOR_LUMA_DEFAULT if luma is None else luma)
    return (colours, feather, luma) if colours else None


def dict2str(opt, indent_level=1):
    msg = ''
    pad = ' ' * (indent_level * 2)
    for k, v in opt.items():
        if isinstance(v, dict):
            msg += f'{pad}{k}:[\n{dict2str(v, indent_level + 1)}{pad}]\n'
        else:
            msg += f'{pad}{k}: {v}\n'
    return msg


def make_exp_dirs(opt):
    """utils/util.py:13-22: raises FileExistsError if results_root exists."""
    os.makedirs(opt['path']['results_root'])


def set_random_seed(seed):
    """utils/util.py:25-31."""
    import random

    import numpy as np
    import torch
    random.seed(seed)
    np.random.seed(seed)
    torch.manual_seed(seed)
    if torch.cuda.is_available():
        torch.cuda.manual_seed(seed)
        torch.cuda.manual_seed_all(seed)
