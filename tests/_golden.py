"""Fixtures under ``tests/golden/``: the reference project's bundled example transcript (xz-compressed JSON)
and, for the cases of the differential tests, what the reference's preprocessor and chunker return -- recorded
once by ``tools/record_reference_golden.py`` as the number of records and the sha256 of their JSON text
(``digest``), so the suite needs nothing outside the repository and the files stay small.  Equal digests are
equal outputs."""
import hashlib
import json
import lzma
import os

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
EXAMPLE = os.path.join(GOLDEN, "transcript-example.json.xz")
RESULTS = os.path.join(GOLDEN, "reference_results.json")

# the cases of tests/test_preprocess.py: (first N segments of the example, keyword arguments)
PREPROCESS_EXAMPLE_SEGMENTS = 1500
PREPROCESS_CASES = [{}, {"time_interval_seconds": 60}, {"time_interval_seconds": 300},
                    {"merge_same_speaker": False, "time_interval_seconds": 120},
                    {"max_segment_duration": 45, "preserve_timestamps": False}]
# the synthetic multi-speaker transcript: utils/synth.py synthetic_transcript(1.0, seed=3, n_speakers=3)
PREPROCESS_SYNTH = {"hours": 1.0, "seed": 3, "n_speakers": 3}
PREPROCESS_SYNTH_CASES = [{}, {"time_interval_seconds": 90}]
# the cases of tests/test_chunker.py: the first N segments, preprocessed, chunked at each token budget
CHUNKER_EXAMPLE_SEGMENTS = 2500
CHUNKER_PREPROCESS = {"max_segment_duration": 600}
CHUNKER_BUDGETS = [600, 2000, 4000]


def key(kwargs) -> str:
    return json.dumps(kwargs, sort_keys=True)


def load_example():
    with lzma.open(EXAMPLE, "rt", encoding="utf-8") as f:
        return json.load(f)


def load_results():
    with open(RESULTS, encoding="utf-8") as f:
        return json.load(f)


def _speakers_sorted(rec):
    """The reference joins the SET of an interval's speakers (``", ".join(set)``), and so does this project: the
    order of the names is the set's iteration order, which string-hash randomisation changes from process to
    process.  A recording made in another process can only be compared with the names in a fixed order."""
    if isinstance(rec.get("speaker"), str):
        rec = dict(rec, speaker=", ".join(sorted(rec["speaker"].split(", "))))
    return rec


def digest(result):
    """{"n": number of records, "sha256": of the records' JSON text} of a list of segments or chunks."""
    text = json.dumps([_speakers_sorted(r) for r in result], sort_keys=True, ensure_ascii=False)
    return {"n": len(result), "sha256": hashlib.sha256(text.encode("utf-8")).hexdigest()}


def assert_same(mine, recorded) -> None:
    """``mine`` (a live result) equals the reference result whose digest was recorded."""
    got = digest(mine)
    assert got["n"] == recorded["n"], "%d records, the reference returned %d" % (got["n"], recorded["n"])
    assert got["sha256"] == recorded["sha256"], "records differ from the reference's (recorded sha256)"
