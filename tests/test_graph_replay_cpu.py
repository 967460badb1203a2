"""include/wfk.h against the graph-replay table, on the host: every entry whose comment promises that it "allocates
nothing and does not synchronise" has a row in tests/test_gpu_graph_replay.py (tests/graph_replay_table.py: ROWS_OF) or
stands on the documented not-capturable list; the header's "Graph capture" paragraph names the same entries; and the
promise has ONE wording.  A stage added later cannot be left out silently."""
import os
import re

from graph_replay_table import NOT_CAPTURABLE, ROWS_OF

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
# "wfk_a() allocates nothing and does not synchronise" / "wfk_a() and wfk_b() allocate nothing and do not synchronise"
PROMISE = re.compile(r'((?:wfk_\w+\(\)(?:\s*,\s*|\s+and\s+)?)+)\s+allocates?\s+nothing\s+and\s+(?:does|do)\s+not\s+synchronise')


def _header():
    with open(os.path.join(ROOT, 'include', 'wfk.h')) as f:
        text = f.read()
    return re.sub(r'\n\s*\*\s?', ' ', text)              # comment lines joined: a sentence may break anywhere


def promised(text):
    return sorted({name for m in PROMISE.finditer(text) for name in re.findall(r'(wfk_\w+)\(\)', m.group(1))})


def declared(text):
    return set(re.findall(r'\bint\s+(wfk_\w+)\s*\(', text))


def test_the_pattern_reads_both_forms_of_the_sentence():
    text = ('x. wfk_a_apply() allocates nothing and does not synchronise; y.  wfk_b_launch() and wfk_c_apply() allocate '
            'nothing and do not synchronise.  wfk_d(), wfk_e() and wfk_f() allocate nothing and do not synchronise.  '
            'wfk_g() allocates nothing.  An entry that "allocates nothing and does not synchronise" may be captured.')
    assert promised(text) == ['wfk_a_apply', 'wfk_b_launch', 'wfk_c_apply', 'wfk_d', 'wfk_e', 'wfk_f']


def test_every_promise_of_the_header_has_a_row():
    text = _header()
    names = promised(text)
    rows = {e for entries in ROWS_OF.values() for e in entries}
    print('promised:', names)
    assert len(names) >= 15 and set(names) <= declared(text), sorted(set(names) - declared(text))
    missing = [n for n in names if n not in rows and n not in NOT_CAPTURABLE]
    assert not missing, f'promised in include/wfk.h, without a row in the graph-replay table: {missing}'
    assert not set(names) & set(NOT_CAPTURABLE), 'an entry cannot promise and be documented as not capturable'
    unpromised = sorted(rows - set(names))
    assert not unpromised, f'in the table, but the header does not promise it: {unpromised}'


def test_the_promise_has_one_wording():
    """every sentence of the header about allocation or synchronisation inside an apply is the pattern's"""
    text = _header()
    loose = re.findall(r'[^.;]*\b(?:no allocation|no host sync|allocates? nothing|not synchroni[sz]e)\b[^.;]*', text)
    odd = [s.strip() for s in loose if not PROMISE.search(s) and 'in these words' not in s]
    assert not odd, odd


def test_the_graph_capture_paragraph_names_the_same_entries():
    text = _header()
    at = text.index('Graph capture.')
    paragraph = text[at:text.index('*/', at)]
    listed = set(re.findall(r'\b(wfk_\w+)\b', paragraph[:paragraph.index('Creation, destruction')]))
    assert listed == set(promised(text)), (sorted(listed ^ set(promised(text))))
    for name in NOT_CAPTURABLE:
        assert name in paragraph, f'{name} is on the not-capturable list but the header does not say so'
