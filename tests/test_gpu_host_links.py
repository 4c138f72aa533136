"""ResidentPagerank.SetLinkKey / TopLinks (host/ranking.hpp): the links of a page by doc hash on the crawl-shaped MemDB corpus of
tests/test_gpu_host.py, against tests/links_model.py built from forw[2] and the forw[3] ranks the Run wrote."""
import json

import numpy as np
import pytest

from tests import links_model as lm
from tests.test_gpu_host import corpus, h, host, make_tables  # noqa: F401  (fixtures)

pytestmark = pytest.mark.gpu


def model_of(pr, forw, children, topic):
    names = list(pr.name)
    idx = {k: i for i, k in enumerate(names)}
    rows = [[idx[c] for c in children.get(k, [])] for k in names]
    ptr = np.zeros(len(names) + 1, dtype=np.uint64)
    ptr[1:] = np.cumsum([len(r) for r in rows])
    dst = np.array([c for r in rows for c in r], dtype=np.uint32)
    key = None if topic is None else np.array([json.loads(forw[3].get(k))[topic] for k in names])
    return names, idx, ptr, dst, key


def check(pr, forw, children, topic, hashes, m):
    names, idx, ptr, dst, key = model_of(pr, forw, children, topic)
    nodes = [idx.get(x, len(names) + 3) for x in hashes]
    for d in (lm.PARENTS, lm.CHILDREN):
        links, degree = pr.TopLinks(hashes, d, m)
        wl, wn, wd = lm.top_links(len(names), ptr, dst, key, d, nodes, m)
        assert [[names[u] for u in wl[i, :wn[i]]] for i in range(len(hashes))] == links
        assert list(degree) == wd.tolist()
    return links, degree


def test_top_links_by_hash(host, corpus):
    forw, inv = make_tables(host, corpus)
    doc = corpus["doc"]
    children = dict(corpus["children"])
    pr = host.ResidentPagerank()
    pr.Build(forw)
    unknown = h("http://elsewhere/not-a-node")
    assert unknown not in pr.name
    hashes = [x for x in doc[:300] if x in pr.name] + [unknown] + list(pr.name[-40:]) + [unknown, pr.name[0], pr.name[0]]
    check(pr, forw, children, None, hashes, 5)                  # no key yet: ascending node id
    with pytest.raises(RuntimeError):
        pr.SetLinkKey("Science")                                # no Run yet: no rank row
    pr.Run(0.75, 1e-9, forw)
    for topic in ("Science", "Arts"):
        pr.SetLinkKey(topic)
        links, degree = check(pr, forw, children, topic, hashes, 5)
    at = hashes.index(unknown)
    assert links[at] == [] and degree[at] == 0
    check(pr, forw, children, "Arts", hashes, 64)
    pr.SetLinkKey("")
    check(pr, forw, children, None, hashes, 5)
    # a re-crawled page links elsewhere and to a page never seen: the resident graph is patched, the key is gone with the old ranks
    page = next(p for p in sorted(children) if len(children[p]) >= 3)
    newcomer = h("http://site/newcomer-for-links")
    children[page] = children[page][:2] + [newcomer, doc[3], doc[3]]
    forw[2].set(page, json.dumps(children[page]))
    pr.SetLinkKey("Arts")
    pr.ApplyDelta(forw, [page])
    if pr.rebuilds == 0:
        assert newcomer in pr.name
    hashes2 = hashes + [page, newcomer, doc[3]]
    check(pr, forw, children, None, hashes2, 5)
    with pytest.raises(RuntimeError):
        pr.SetLinkKey("Arts")                                   # the rank rows of the old node set are no key for the new one
    pr.Run(0.75, 1e-9, forw)
    pr.SetLinkKey("Sports")
    links, degree = check(pr, forw, children, "Sports", hashes2, 5)
    assert degree[len(hashes)] == 5 and links[len(hashes) + 1] == []
    assert page in pr.TopLinks([newcomer], lm.PARENTS, 5)[0][0]
