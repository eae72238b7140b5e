// nwt_map.hpp -- the map of the memory of the structured Newton mode (newton.hpp) and the QP-based SQP step (qpdual.hpp) of sqp_kernel.  The host
// sizes the workspace (plan_solve.cpp, nwt_doubles) and the LDS area (layout.cpp, ntg_make_layout) from it.  sqp_kernel computes the same offsets in its
// prologue (nwt_ksz, qp_pp, nwt_yall, qpbase, ...: DESIGN.md section 2 says why they stay there); whoever changes one side changes the other.
// Plain host / device code: tests/drivers/nwt_map_drv.cpp prints it for a table of shapes.
#pragma once
#include <stddef.h>
#include "qpdual.hpp"

#define NWT_PANEL 416    // LDS doubles a factoring wave owns (nwt_factor_wave: two buffers of four panel columns, stride 52)
#define NWT_STAGE 216    // LDS doubles a wave of the assembly owns (nwt_assemble: the blocks of one knot interval, staged)

struct NwtMap {
	// Per-problem workspace (HBM), offsets in doubles.  From 0 the groups' band arrays [ngrp][ng][hb + 1]; Kb: the reversed arrays of the
	// two-sided factorisation [ngrp][16 jb + 48][hb + 1]; B: the per-breakpoint blocks [ngrp][P][cg cg]; QP step: the slots' columns
	// U = W J' [qa][npad] and, per row (ncq = ncnln rounded up to even), the QP's multipliers of the previous major (lamq), c, J W g, the
	// derivative rows a [cg] and J U [qa].
	size_t Kb, B, U, lamq, c, jwg, a, JU, total, npad, ncq;
	// The LDS area at SmemLayout::nwt_y, offsets in doubles.  Between refreshes: from 0 the groups' solve vectors [ngrp][ylen] -- two-sided
	// their top parts with the separator [ngrp][lena], from yb the reversed rest [ngrp][lenb]; panel: [npan][NWT_PANEL], one per factoring wave;
	// yf: the free outputs' vectors [nfo][ylenf]; QP step: slots [ngrp][qpd] (qa slots per group), red [NTG_QP_RED] scratch of the entering-row
	// search.  Inside a refresh instead: from 0 the assembly's staging buffers [waves][NWT_STAGE], from act the block-flag words
	// [ngrp][(P + 63) / 64].  bytes: size of the area.
	int ylen, lena, lenb, yb, panel, npan, yf, ylenf, qa, qpd, slots, red, act, bytes;
	// the reduction scratch (SmemLayout::red): its doubles, and the int index of the mode's flag word pair (its last two words)
	int red_doubles, flag;
};

// D: NtgDims (or anything with its nC, ncnln, P and nwt_* members); cg: Family::CG (= NtgDims::nwt_cg on the host)
template <class DIMS>
NTG_HD NwtMap nwt_map(const DIMS &D, int nthreads, int qp, int cg)
{
	NwtMap m;
	const int ngrp = D.nwt_ngrp, waves = nthreads / 64;
	m.npad = (size_t)((D.nC + 1) & ~1); m.ncq = (size_t)((D.ncnln + 1) & ~1);
	m.qa = ntg_qp_maxa(ngrp, nthreads); m.qpd = ntg_qp_doubles(m.qa);
	m.Kb = (size_t)ngrp * D.nwt_ng * (D.nwt_hb + 1);
	m.B = m.Kb + (D.nwt_tw ? (size_t)ngrp * (16 * D.nwt_jb + 48) * (D.nwt_hb + 1) : 0);
	m.U = m.B + (size_t)ngrp * D.P * cg * cg;
	m.lamq = m.U + (qp ? (size_t)m.qa * m.npad : 0);
	m.c = m.lamq + (qp ? m.ncq : 0); m.jwg = m.c + (qp ? m.ncq : 0); m.a = m.jwg + (qp ? m.ncq : 0);
	m.JU = m.a + (qp ? m.ncq * cg : 0); m.total = m.JU + (qp ? m.ncq * m.qa : 0);
	m.ylen = 16 * ((D.nwt_ng + 15) >> 4) + 48; m.lena = 16 * (D.nwt_ja + 3) + 48; m.lenb = 16 * (D.nwt_jb + 3) + 48;
	m.yb = ngrp * m.lena; m.panel = ngrp * (D.nwt_tw ? m.lena + m.lenb : m.ylen); m.npan = (D.nwt_tw ? 2 : 1) * ngrp;
	m.yf = m.panel + m.npan * NWT_PANEL; m.ylenf = 16 * ((D.nwt_ngf + 15) >> 4) + 48;
	m.slots = m.yf + D.nwt_nfo * m.ylenf; m.red = m.slots + ngrp * m.qpd; m.act = waves * NWT_STAGE;
	const int steady = qp ? m.red + NTG_QP_RED : m.slots, refresh = m.act + ngrp * ((D.P + 63) / 64);
	m.bytes = (steady > refresh ? steady : refresh) * 8;
	m.red_doubles = 32 * waves + 2; m.flag = 2 * m.red_doubles - 2;
	return m;
}
