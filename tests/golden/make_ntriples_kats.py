#!/usr/bin/env python3
"""Writes tests/golden/ntriples_kats.json: N-Triples fixtures of the reference's parser test suite with their outcome, transcribed by
hand as DATA (the fixture's text, and what its manifest says of it: the triples, or that it is refused and on which line).

Sources (relative to the rdf-fusion tree, testsuite/):
  oxigraph-tests/parser/manifest.ttl        no_end_line_jump (TestNTriplesPositiveSyntax); escaped_trailing_dot, at_keywords_as_lang_tag,
                                            language_normalization, literal_value_space: the .nt files are the expected RESULTS of Turtle /
                                            RDF-XML evaluation tests, which the test runner loads with the N-Triples parser
  serd-tests/good/manifest.ttl              test-blankdot
  oxigraph-tests/parser-error/manifest.ttl  invalid_iri, invalid_iri_crlf, invalid_iri_comment, invalid_predicate, invalid_string_escape,
                                            unexpected_eof (negative syntax tests; the line is where the fixture goes wrong)
No other .nt file of those directories is taken: many are outputs of Turtle tests or belong to the unchecked / recovery modes.

A term is [kind, lexical form, suffix]: kind 1 IRI, 2 blank node, 3 simple literal, 4 language-tagged literal (suffix = the tag in lower
case), 5 typed literal (suffix = the datatype IRI)."""
import json
import os

I = lambda s: [1, s, ""]
EX = "http://example.com"
RDF_VALUE = "http://www.w3.org/1999/02/22-rdf-syntax-ns#value"
_INVALID_IRI = "<http://example.com/s> <http://example.com/p> <http://example.com/o> .\n<http://example.com/s> <http:// /p> <http://example.com/o> .\n"

fixtures = [
    dict(file="oxigraph-tests/parser/no_end_line_jump.nt",
         text="<http://example.com> <http://example.com> <http://example.com> .",
         triples=[[I(EX), I(EX), I(EX)]]),
    dict(file="oxigraph-tests/parser/escaped_trailing_dot.nt",
         text="<http://example.com/s> <http://example.com/p> <http://example.com/o.> .\n",
         triples=[[I(EX + "/s"), I(EX + "/p"), I(EX + "/o.")]]),
    dict(file="oxigraph-tests/parser/at_keywords_as_lang_tag.nt",
         text='<http://example.com/s> <http://example.com/p> "foo"@base .\n<http://example.com/s> <http://example.com/p> "bar"@prefix .\n',
         triples=[[I(EX + "/s"), I(EX + "/p"), [4, "foo", "base"]], [I(EX + "/s"), I(EX + "/p"), [4, "bar", "prefix"]]]),
    dict(file="oxigraph-tests/parser/language_normalization.nt",
         text='<http://foo> <http://foo> "foo"@en-us .',
         triples=[[I("http://foo"), I("http://foo"), [4, "foo", "en-us"]]]),
    dict(file="oxigraph-tests/parser/literal_value_space.nt",
         text='<http://example.com/foo> <%s> "  bar\\n" .\n' % RDF_VALUE,
         triples=[[I(EX + "/foo"), I(RDF_VALUE), [3, "  bar\n", ""]]]),
    dict(file="serd-tests/good/test-blankdot.nt",
         text="<http://example.org/subject> <http://example.org/predicate> _:c .\n",
         triples=[[I("http://example.org/subject"), I("http://example.org/predicate"), [2, "c", ""]]]),
    dict(file="oxigraph-tests/parser-error/invalid_iri.nt", text=_INVALID_IRI, refused_line=2),
    dict(file="oxigraph-tests/parser-error/invalid_iri_crlf.nt", text=_INVALID_IRI, refused_line=2,
         note="the fixture's bytes are those of invalid_iri.nt: it holds LF line ends"),
    dict(file="oxigraph-tests/parser-error/invalid_iri_comment.nt",
         text="<http://example.com/s> <http://example.com/p> <http://example.com/o> . # foo\n<http://example.com/s> <http:// /p> <http://example.com/o> .\n",
         refused_line=2),
    dict(file="oxigraph-tests/parser-error/invalid_predicate.nt",
         text='<http://example.com/s> <http://example.com/p> <http://example.com/o> .\n<http://example.com/s> "p" <http://example.com/o> .\n',
         refused_line=2),
    dict(file="oxigraph-tests/parser-error/invalid_string_escape.nt",
         text='<http://example.com/s> <http://example.com/p> "fooé \\a baré" .\n', refused_line=1),
    dict(file="oxigraph-tests/parser-error/unexpected_eof.nt",
         text="<http://example.com/s> <http://example.com/p> <http://example.com/o\nbé", refused_line=1),
]

out = dict(_about="N-Triples fixtures of the reference's parser test suite with their outcome (see make_ntriples_kats.py).", fixtures=fixtures)

if __name__ == "__main__":
    path = os.path.join(os.path.dirname(os.path.abspath(__file__)), "ntriples_kats.json")
    with open(path, "w") as f:
        json.dump(out, f, indent=1)
    print("wrote", path)
