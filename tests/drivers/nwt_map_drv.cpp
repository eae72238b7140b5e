// Host print-out of csrc/nwt_map.hpp (the memory map of the structured Newton mode and the QP-based SQP step) for a table of shapes; built
// with g++ and checked by tests/test_nwt_map.py against the three formulas the map replaced.  One line per (shape, nthreads, qp): the
// inputs, then every member of the map.
#include <cstdio>
#include "../../ntg_amd/csrc/nwt_map.hpp"

struct Dims { int nC, ncnln, P, nwt_ngrp, nwt_ng, nwt_hb, nwt_tw, nwt_ja, nwt_jb, nwt_nfo, nwt_ngf, cg; };

int main()
{
	// one group / several groups, two-sided on / off, with / without free outputs, odd nC and ncnln, a P that is no multiple of 64
	const Dims shapes[] = {
		{126, 101, 101, 1, 114, 11, 0, 0, 0, 0, 0, 2},        // the obstacle class: one group, small
		{127, 63, 21, 1, 40, 11, 0, 0, 0, 0, 0, 2},           // odd nC, odd ncnln
		{172, 42, 21, 1, 123, 23, 0, 0, 0, 1, 37, 4},         // one group and a free output
		{616, 402, 201, 1, 462, 23, 1, 13, 13, 1, 150, 4},    // two-sided, free output
		{531, 129, 129, 1, 531, 17, 1, 16, 15, 0, 0, 3},      // two-sided, ja != jb, odd everything
		{732, 122, 61, 2, 180, 11, 0, 0, 0, 0, 0, 3},         // two groups
		{2196, 1204, 301, 4, 543, 17, 0, 0, 0, 0, 0, 3},      // four groups (the BIG layout's size)
		{1098, 301, 301, 2, 300, 17, 1, 8, 8, 2, 65, 6},      // two groups, two-sided, two free outputs, the largest block
	};
	for (const Dims &d : shapes)
		for (int nt = 128; nt <= 512; nt *= 2)
			for (int qp = 0; qp < 2; qp++) {
				const NwtMap m = nwt_map(d, nt, qp, d.cg);
				printf("%d %d %d %d %d %d %d %d %d %d %d %d %d %d", d.nC, d.ncnln, d.P, d.nwt_ngrp, d.nwt_ng, d.nwt_hb, d.nwt_tw, d.nwt_ja, d.nwt_jb, d.nwt_nfo, d.nwt_ngf, d.cg, nt, qp);
				printf(" %zu %zu %zu %zu %zu %zu %zu %zu %zu %zu %zu", m.Kb, m.B, m.U, m.lamq, m.c, m.jwg, m.a, m.JU, m.total, m.npad, m.ncq);
				printf(" %d %d %d %d %d %d %d %d %d %d %d %d %d %d %d %d\n", m.ylen, m.lena, m.lenb, m.yb, m.panel, m.npan, m.yf, m.ylenf, m.qa, m.qpd, m.slots, m.red, m.act, m.bytes, m.red_doubles, m.flag);
			}
	return 0;
}
