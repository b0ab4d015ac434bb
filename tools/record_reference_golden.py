#!/usr/bin/env python3
"""Record what the reference project's preprocessor and chunker return for the cases of the differential
tests (tests/test_preprocess.py, tests/test_chunker.py) into tests/golden/, together with an xz-compressed
copy of its bundled example transcript, so the suite runs without the reference checkout.

    python tools/record_reference_golden.py --reference /path/to/reference/checkout

The reference modules are loaded from that checkout and only run; nothing of their code is stored.  The
chunker gets this project's tokenizer and sentence splitter injected in place of tiktoken / nltk, as the
differential test always did (same tokenizer on both sides: identical chunks).  Results are stored as
record counts and sha256 digests (tests/_golden.py digest)."""
import argparse
import contextlib
import importlib.util
import io
import json
import lzma
import os
import sys
import types

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import _golden as G  # noqa: E402


def _load(path: str, name: str):
    spec = importlib.util.spec_from_file_location(name, path)
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def _load_chunker(path: str):
    from llm_map_reduce_summarizer_amd.engine.tokenizer import get_tokenizer
    from llm_map_reduce_summarizer_amd.pipeline.chunker import split_sentences
    tok = get_tokenizer()

    class Enc:
        def encode(self, text):
            return tok.encode_ordinary(text)

    class Punkt:
        def tokenize(self, text):
            return split_sentences(text)

    fake_nltk = types.ModuleType("nltk")
    fake_nltk.data = types.SimpleNamespace(find=lambda *_: True)
    fake_nltk.tokenize = types.SimpleNamespace(PunktSentenceTokenizer=Punkt)
    sys.modules["nltk"] = fake_nltk
    sys.modules["tiktoken"] = types.SimpleNamespace(get_encoding=lambda name: Enc())
    return _load(path, "ref_chunker")


def main() -> int:
    ap = argparse.ArgumentParser()
    ap.add_argument("--reference", required=True, help="checkout of the reference project")
    a = ap.parse_args()
    from llm_map_reduce_summarizer_amd.pipeline.preprocess import preprocess_transcript
    from llm_map_reduce_summarizer_amd.utils.synth import synthetic_transcript

    os.makedirs(G.GOLDEN, exist_ok=True)
    with open(os.path.join(a.reference, "transcript-example.json"), encoding="utf-8") as f:
        example = json.load(f)
    with lzma.open(G.EXAMPLE, "wt", encoding="utf-8", preset=9 | lzma.PRESET_EXTREME) as f:
        json.dump(example, f, separators=(",", ":"), ensure_ascii=False)  # same content, no whitespace

    pre = _load(os.path.join(a.reference, "preprocessor.py"), "ref_preprocessor")
    chunker = _load_chunker(os.path.join(a.reference, "big_chunkeroosky.py"))
    with contextlib.redirect_stdout(io.StringIO()):  # the reference prints its progress
        segs = example["segments"][:G.PREPROCESS_EXAMPLE_SEGMENTS]
        synth = synthetic_transcript(**G.PREPROCESS_SYNTH)["segments"]
        rec = {"preprocess_example": {G.key(kw): G.digest(pre.preprocess_transcript(segs, **kw))
                                      for kw in G.PREPROCESS_CASES},
               "preprocess_synthetic": {G.key(kw): G.digest(pre.preprocess_transcript(synth, **kw))
                                        for kw in G.PREPROCESS_SYNTH_CASES},
               "chunks": {}}
        segs = preprocess_transcript(example["segments"][:G.CHUNKER_EXAMPLE_SEGMENTS], **G.CHUNKER_PREPROCESS)
        for budget in G.CHUNKER_BUDGETS:
            r = chunker.BigChunkeroosky(max_tokens_per_chunk=budget)
            rec["chunks"][str(budget)] = G.digest(r.postprocess_chunks(r.chunk_transcript(segs)))
    with open(G.RESULTS, "w", encoding="utf-8") as f:
        json.dump(rec, f, indent=1, sort_keys=True)
        f.write("\n")
    for p in (G.EXAMPLE, G.RESULTS):
        print("%s: %d bytes" % (os.path.relpath(p, ROOT), os.path.getsize(p)))
    return 0


if __name__ == "__main__":
    sys.exit(main())
