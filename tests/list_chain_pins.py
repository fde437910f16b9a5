"""What the host tests of the five list records pin of the source text (csrc/report_sections.h, csrc/ctx.h): one enum in the order the sections
ride, one definition of each piece of the section arithmetic, one store array, and none of the names the side mechanisms of the transfer records
and the delivered rows' records had."""
import glob
import os
import re

ENUM = "enum { LIST_FIT, LIST_GRAM, LIST_TAPFIT, LIST_TRANSFER, LIST_DELIVERED, LIST_KINDS };"
ONCE = ["static inline ListSection list_section(", "static inline size_t list_room(", "static inline ListSections list_sections(", "static inline size_t lists_room("]
GONE = ["transfer_section", "delivered_section", "transfer_rec", "delivered_rec", "transfer_begin", "delivered_begin"]


def assert_one_chain(csrc):
    text = {}
    for path in sorted(glob.glob(os.path.join(csrc, "*"))):
        if os.path.splitext(path)[1] in (".h", ".cpp", ".hip") or os.path.basename(path) == "Makefile":
            with open(path) as f:
                text[os.path.basename(path)] = f.read()
    sections = text["report_sections.h"]
    assert ENUM in sections                                                      # the five kinds, in the order the sections ride
    for definition in ONCE:
        assert sections.count(definition) == 1, definition
        assert sum(t.count(definition) for t in text.values()) == 1, definition
    for name in GONE:
        found = [f for f, t in text.items() if re.search(r"\b%s\b" % name, t)]
        assert not found, (name, found)
    assert "list_rec[LIST_KINDS]" in text["ctx.h"]                               # one store per kind, all five
    assert "list_sections(" in text["api_batch.cpp"] and "lists_room(" in text["api_batch.cpp"]
