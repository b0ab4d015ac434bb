"""Configuration from the environment / ``.env`` (layer L0).

Reference: ``LLMConfig`` class attributes read once at import
(``llm_executor.py:31-52``) after ``load_dotenv()`` (``:29``, ``main.py:43``);
keys documented in ``.env.template:1-22``.

Here the same keys are recognised (plus engine keys), a minimal ``.env``
reader replaces python-dotenv (not installed offline; existing environment
variables win, as with ``load_dotenv(override=False)``), and an
``LLMConfig()`` *instance* re-reads the environment so settings changed after
import take effect (reference values stay available as class attributes).
Defaults follow the code / ``.env.template``, not the README.
"""

from __future__ import annotations

import os
from typing import Optional

_DOTENV_LOADED = False


def load_dotenv(path: Optional[str] = None) -> bool:
    """Populate ``os.environ`` from ``KEY=VALUE`` lines (inline ``#`` comments stripped)."""
    global _DOTENV_LOADED
    path = path or os.path.join(os.getcwd(), ".env")
    if not os.path.isfile(path):
        return False
    with open(path, "r", encoding="utf-8") as f:
        for raw in f:
            line = raw.strip()
            if not line or line.startswith("#") or "=" not in line:
                continue
            key, val = line.split("=", 1)
            key = key.strip()
            if key.startswith("export "):
                key = key[7:].strip()
            val = val.strip()
            if val[:1] in "\"'" and val[-1:] == val[:1] and len(val) >= 2:
                val = val[1:-1]
            elif " #" in val:
                val = val.split(" #", 1)[0].rstrip()
            os.environ.setdefault(key, val)
    _DOTENV_LOADED = True
    return True


def _env(key: str, default: str) -> str:
    return os.environ.get(key, default)


def parse_logit_bias(spec: str):
    """``"ID:BIAS,ID:BIAS"`` ($LOGIT_BIAS / --logit-bias) as [(token id, bias)]; a BIAS written ``ban`` is
    -inf.  Raises ValueError for anything else, a repeated id and a bias outside [-100, 100] included."""
    out = []
    for part in (x.strip() for x in spec.split(",")):
        if not part:
            continue
        tok, sep, bias = part.partition(":")
        try:
            if not sep:
                raise ValueError
            t = int(tok.strip())
            x = float("-inf") if bias.strip().lower() == "ban" else float(bias)
        except ValueError:
            raise ValueError("logit bias entry %r is not ID:BIAS (BIAS a number or 'ban')" % part) from None
        if t < 0 or not (x == float("-inf") or -100.0 <= x <= 100.0):  # (NaN fails the range)
            raise ValueError("logit bias entry %r needs an id >= 0 and a bias in [-100, 100] or 'ban'" % part)
        out.append((t, x))
    if len({t for t, _ in out}) != len(out):
        raise ValueError("logit bias %r names a token twice" % spec)
    if len(out) > 300:
        raise ValueError("logit bias holds %d entries, at most 300 are allowed" % len(out))
    return out


class LLMConfig:
    """Provider + generation settings.  Class attributes = values at import time."""

    _FIELDS = {
        "OPENAI_API_KEY": ("", str), "OPENAI_ORG_ID": ("", str), "OPENAI_MODEL": ("gpt-3.5-turbo", str),
        "ANTHROPIC_API_KEY": ("", str), "ANTHROPIC_MODEL": ("claude-3-sonnet-20240229", str),
        "MAX_CONCURRENT_REQUESTS": ("5", int), "TEMPERATURE": ("0.3", float), "MAX_TOKENS": ("1000", int),
        "REQUEST_TIMEOUT": ("60", int), "RETRY_ATTEMPTS": ("3", int), "RETRY_DELAY": ("5", float),
        "DEFAULT_PROVIDER": ("local", str),
        # engine (new)
        "LOCAL_MODEL": ("llama3-8b", str), "ENGINE_DTYPE": ("bf16", str), "ENGINE_SEED": ("0", int),
        "ENGINE_MAX_NUM_SEQS": ("256", int), "ENGINE_KV_FRACTION": ("0.6", float),
        "ENGINE_KV_DTYPE": ("bf16", str),
        # KV prefix cache of the local engines: prompts that begin with the same tokens share pages (1 = on)
        "ENGINE_PREFIX_CACHE": ("0", int),
        "REDUCE_TEMPERATURE": ("0.2", float),
        # sampling filters of the map and the reduce stage (1.0 / 0 = off)
        "TOP_P": ("1.0", float), "TOP_K": ("0", int),
        # penalties on the tokens a sequence has generated, map and reduce (0 / 0 / 1 = off)
        "FREQUENCY_PENALTY": ("0.0", float), "PRESENCE_PENALTY": ("0.0", float),
        "REPETITION_PENALTY": ("1.0", float),
        # constraints, map and reduce: fewest tokens before a stop id can be sampled (0 = off) and a logit bias
        # "ID:BIAS,ID:BIAS" over the local tokenizer's ids, BIAS in [-100, 100] or "ban" (empty = off)
        "MIN_NEW_TOKENS": ("0", int), "LOGIT_BIAS": ("", str),
        # hosted-provider endpoints (new): point the adapters at any compatible server
        "OPENAI_BASE_URL": ("https://api.openai.com/v1", str),
        "ANTHROPIC_BASE_URL": ("https://api.anthropic.com/v1", str),
    }

    def __init__(self, **overrides):
        for k, (d, typ) in self._FIELDS.items():
            setattr(self, k, typ(_env(k, d)))
        for k, v in overrides.items():
            if k not in self._FIELDS:
                raise TypeError("unknown config key %s" % k)
            setattr(self, k, v)

    def api_key(self, provider: str) -> str:
        return {"openai": self.OPENAI_API_KEY, "anthropic": self.ANTHROPIC_API_KEY}.get(provider, "")


load_dotenv()
for _k, (_d, _t) in LLMConfig._FIELDS.items():
    setattr(LLMConfig, _k, _t(_env(_k, _d)))
