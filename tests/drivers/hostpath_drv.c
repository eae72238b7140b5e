/*
 * tests/drivers/hostpath_drv.c -- the host-callback path of the drop-in (include/ntg.h, include/ntg_amd.h) on problems read from a
 * text file: every flat output with its own order, mult, maxderiv and knot vector, linear rows of all three kinds, and HOST callbacks
 * in all six slots.  Written against the two public headers only, so the same source links against the oracle's ABI library and
 * against the product (tests/test_hostpath_oracle.py, tests/test_gpu_hostpath.py); tests/hostpath_cases.py writes the files.
 *
 * Problem file (tokens separated by white space, key words checked):
 *   NOUT n            then per output: order mult maxderiv ninterv knot_0 .. knot_ninterv
 *   BPS P             then the P breakpoints
 *   LIC n / LTC n / LFC n   each followed by n rows of nz = sum(maxderiv) entries
 *   AV                six lists "count (output deriv)*": icav tcav fcav icostav tcostav fcostav
 *   NFUNC             nnlic nnltc nnlfc nicf nucf nfcf
 *   BOUNDS nb         lower[nb] upper[nb]
 *   FUNCS             per slot (nlic, nltc, nlfc, icf, ucf, fcf) and per function of it, over the slot's list u_0 .. u_{n-1}:
 *                     a[n] b[n]   nbil (p q w)*   nsin (p w s)*
 *   COEF nC values    the initial guess of a solve
 *   POINTS npts       per point: full (1: everything, 0: F and C in mode 0 only) and nC coefficients
 *   TIMES nt          the interpolation times
 *
 * The callbacks take the reference's callback ABI (ntg.h:81-83,90-92) and read only zp[o][r].  Every function of every slot is
 *   f(u) = sum_j (a_j u_j^2 + b_j u_j) + sum_e w_e u_{p_e} u_{q_e} + sum_e w_e sin(s_e u_{p_e})
 * over the slot's declared active variables u_j = zp[o_j][r_j]; df / dc are written over all nz entries, zero outside the list.
 *
 * Usage:
 *   hostpath_drv eval FILE                      ntg_open(); per point: F, G (mode 2), F0 (mode 0), G1 (mode 1), C and J (mode 2, ldJ =
 *                                               ncnln + 2 on a buffer filled with -7.25), Z lines (what the trajectory cost callback
 *                                               was handed for its list at every breakpoint) and INTERP lines (SplineInterp of every
 *                                               output with its own maxderiv at the times); all numbers %.17g
 *   hostpath_drv solve FILE [option]...         npsoloption(option)..., ntg(): "RESULT inform objective coef...", "ISTATE" of the
 *                                               linear rows; ntg() prints its exit line itself.  Exit status: inform.
 *   hostpath_drv sequence FILE1 FILE2 [option]...   solve FILE1, FILE2, FILE1 in one process
 */
#include <math.h>
#include "ntg.h"
#include "ntg_amd.h"

typedef struct { int n; AV *av; int *flat; } List;   /* flat[j] = iz[output] + deriv */
typedef struct { double *a, *b; int nbil, *bp, *bq; double *bw; int nsin, *sp; double *sw, *ss; } Func;
typedef struct {
	int nout, nz, nC, nbps, *order, *mult, *md, *nint, *ncoef, *iC, *iz;
	double **knots, *bps;
	int nlin[3]; double **lin[3];
	List L[6]; int nf[6]; Func *F[6];      /* slots: 0 nlic, 1 nltc, 2 nlfc, 3 icf, 4 ucf, 5 fcf */
	int nb; double *lo, *up, *coef;
	int npts, *full; double **pts;
	int ntimes; double *times;
} Prob;

static Prob *G;            /* the problem the callbacks serve */
static double *g_rec;      /* [nbps][L[4].n]: what the trajectory cost callback was handed, when recording */
static FILE *fp;

static void die(const char *what) { fprintf(stderr, "hostpath_drv: %s\n", what); exit(2); }
static int ri(void) { int v; if (fscanf(fp, "%d", &v) != 1) die("integer expected"); return v; }
static double rd(void) { double v; if (fscanf(fp, "%lf", &v) != 1) die("number expected"); return v; }
static void key(const char *k) { char b[32]; if (fscanf(fp, "%31s", b) != 1 || strcmp(b, k)) die(k); }
static double *rdv(int n) { double *v = calloc(n > 0 ? n : 1, sizeof(double)); int i; for (i = 0; i < n; i++) v[i] = rd(); return v; }

static Prob *read_problem(const char *path)
{
	static const char *lk[3] = {"LIC", "LTC", "LFC"};
	Prob *p = calloc(1, sizeof(*p)); int o, s, i, j;
	fp = fopen(path, "r"); if (!fp) die("cannot open the problem file");
	key("NOUT"); p->nout = ri();
	p->order = calloc(p->nout, sizeof(int)); p->mult = calloc(p->nout, sizeof(int)); p->md = calloc(p->nout, sizeof(int));
	p->nint = calloc(p->nout, sizeof(int)); p->ncoef = calloc(p->nout, sizeof(int)); p->iC = calloc(p->nout, sizeof(int));
	p->iz = calloc(p->nout, sizeof(int)); p->knots = calloc(p->nout, sizeof(double *));
	for (o = 0; o < p->nout; o++) {
		p->order[o] = ri(); p->mult[o] = ri(); p->md[o] = ri(); p->nint[o] = ri();
		p->knots[o] = rdv(p->nint[o] + 1);
		p->ncoef[o] = p->nint[o] * (p->order[o] - p->mult[o]) + p->mult[o];
		p->iC[o] = p->nC; p->iz[o] = p->nz; p->nC += p->ncoef[o]; p->nz += p->md[o];
	}
	key("BPS"); p->nbps = ri(); p->bps = rdv(p->nbps);
	for (s = 0; s < 3; s++) {
		key(lk[s]); p->nlin[s] = ri();
		p->lin[s] = DoubleMatrix(p->nlin[s] > 0 ? p->nlin[s] : 1, p->nz);
		for (i = 0; i < p->nlin[s]; i++) for (j = 0; j < p->nz; j++) p->lin[s][i][j] = rd();
	}
	key("AV");
	for (s = 0; s < 6; s++) {
		List *l = &p->L[s];
		l->n = ri(); l->av = calloc(l->n > 0 ? l->n : 1, sizeof(AV)); l->flat = calloc(l->n > 0 ? l->n : 1, sizeof(int));
		for (j = 0; j < l->n; j++) {
			l->av[j].output = ri(); l->av[j].deriv = ri();
			if (l->av[j].output < 0 || l->av[j].output >= p->nout || l->av[j].deriv < 0 || l->av[j].deriv >= p->md[l->av[j].output]) die("active variable out of range");
			l->flat[j] = p->iz[l->av[j].output] + l->av[j].deriv;
		}
	}
	key("NFUNC"); for (s = 0; s < 6; s++) p->nf[s] = ri();
	key("BOUNDS"); p->nb = ri(); p->lo = rdv(p->nb); p->up = rdv(p->nb);
	if (p->nb != p->nlin[0] + p->nlin[1] + p->nlin[2] + p->nf[0] + p->nf[1] + p->nf[2]) die("wrong number of bounds");
	key("FUNCS");
	for (s = 0; s < 6; s++) {
		const int n = p->L[s].n;
		p->F[s] = calloc(p->nf[s] > 0 ? p->nf[s] : 1, sizeof(Func));
		for (i = 0; i < p->nf[s]; i++) {
			Func *f = &p->F[s][i];
			f->a = rdv(n); f->b = rdv(n);
			f->nbil = ri(); f->bp = calloc(f->nbil + 1, sizeof(int)); f->bq = calloc(f->nbil + 1, sizeof(int)); f->bw = calloc(f->nbil + 1, sizeof(double));
			for (j = 0; j < f->nbil; j++) { f->bp[j] = ri(); f->bq[j] = ri(); f->bw[j] = rd(); if (f->bp[j] < 0 || f->bp[j] >= n || f->bq[j] < 0 || f->bq[j] >= n) die("bilinear term out of range"); }
			f->nsin = ri(); f->sp = calloc(f->nsin + 1, sizeof(int)); f->sw = calloc(f->nsin + 1, sizeof(double)); f->ss = calloc(f->nsin + 1, sizeof(double));
			for (j = 0; j < f->nsin; j++) { f->sp[j] = ri(); f->sw[j] = rd(); f->ss[j] = rd(); if (f->sp[j] < 0 || f->sp[j] >= n) die("sin term out of range"); }
		}
	}
	key("COEF"); if (ri() != p->nC) die("COEF: wrong length"); p->coef = rdv(p->nC);
	key("POINTS"); p->npts = ri(); p->full = calloc(p->npts + 1, sizeof(int)); p->pts = calloc(p->npts + 1, sizeof(double *));
	for (i = 0; i < p->npts; i++) { p->full[i] = ri(); p->pts[i] = rdv(p->nC); }
	key("TIMES"); p->ntimes = ri(); p->times = rdv(p->ntimes);
	fclose(fp);
	return p;
}

/* value of one function at zp; d (all nz entries, zero outside the list) when d != NULL */
static double fn_eval(const Func *f, const List *l, double **zp, double *d)
{
	double u[NTG_MAX_NZ], v = 0.0; int j;
	for (j = 0; j < l->n; j++) u[j] = zp[l->av[j].output][l->av[j].deriv];
	if (d) for (j = 0; j < G->nz; j++) d[j] = 0.0;
	for (j = 0; j < l->n; j++) { v += f->a[j] * u[j] * u[j] + f->b[j] * u[j]; if (d) d[l->flat[j]] += 2.0 * f->a[j] * u[j] + f->b[j]; }
	for (j = 0; j < f->nbil; j++) {
		const int p = f->bp[j], q = f->bq[j];
		v += f->bw[j] * u[p] * u[q];
		if (d) { d[l->flat[p]] += f->bw[j] * u[q]; d[l->flat[q]] += f->bw[j] * u[p]; }
	}
	for (j = 0; j < f->nsin; j++) {
		const int p = f->sp[j];
		v += f->sw[j] * sin(f->ss[j] * u[p]);
		if (d) d[l->flat[p]] += f->sw[j] * f->ss[j] * cos(f->ss[j] * u[p]);
	}
	return v;
}
static void cost_slot(int s, int mode, double *f, double *df, double **zp)
{
	const double v = fn_eval(&G->F[s][0], &G->L[s], zp, mode != 0 ? df : NULL);
	if (mode != 1) *f = v;
}
static void con_slot(int s, int mode, double *c, double **dc, double **zp)
{
	int r;
	for (r = 0; r < G->nf[s]; r++) { const double v = fn_eval(&G->F[s][r], &G->L[s], zp, mode != 0 ? dc[r] : NULL); if (mode != 1) c[r] = v; }
}
static void icf(int *mode, int *ns, double *f, double *df, double **zp) { (void)ns; cost_slot(3, *mode, f, df, zp); }
static void ucf(int *mode, int *ns, int *i, double *f, double *df, double **zp)
{
	int j; (void)ns;
	if (g_rec) for (j = 0; j < G->L[4].n; j++) g_rec[(size_t)*i * G->L[4].n + j] = zp[G->L[4].av[j].output][G->L[4].av[j].deriv];
	cost_slot(4, *mode, f, df, zp);
}
static void fcf(int *mode, int *ns, double *f, double *df, double **zp) { (void)ns; cost_slot(5, *mode, f, df, zp); }
static void nlicf(int *mode, int *ns, double *c, double **dc, double **zp) { (void)ns; con_slot(0, *mode, c, dc, zp); }
static void nltcf(int *mode, int *ns, int *i, double *c, double **dc, double **zp) { (void)ns; (void)i; con_slot(1, *mode, c, dc, zp); }
static void nlfcf(int *mode, int *ns, double *c, double **dc, double **zp) { (void)ns; con_slot(2, *mode, c, dc, zp); }

static void pvec(const char *tag, const double *v, size_t n) { size_t j; printf("%s", tag); for (j = 0; j < n; j++) printf(" %.17g", v[j]); printf("\n"); }

static int run_eval(Prob *p)
{
	const int n = p->nC, P = p->nbps, nc = p->nf[0] + p->nf[1] * P + p->nf[2], ldJ0 = nc + 2, nt = p->L[4].n;
	double F, *g = calloc(n, sizeof(double)), *c = calloc(nc + 1, sizeof(double)), *J = calloc((size_t)ldJ0 * n, sizeof(double));
	double *rec = calloc((size_t)P * (nt > 0 ? nt : 1), sizeof(double)), fz[NTG_MAX_ORDER];
	int pt, i, o, t; size_t e;
	G = p;
	if (ntg_open(p->nout, p->bps, P, p->nint, p->knots, p->order, p->mult, p->md, p->nlin[0], p->lin[0], p->nlin[1], p->lin[1], p->nlin[2], p->lin[2],
	             p->nf[0], nlicf, p->nf[1], nltcf, p->nf[2], nlfcf, p->L[0].n, (ntg_av *)p->L[0].av, p->L[1].n, (ntg_av *)p->L[1].av, p->L[2].n, (ntg_av *)p->L[2].av,
	             p->nf[3], icf, p->nf[4], ucf, p->nf[5], fcf, p->L[3].n, (ntg_av *)p->L[3].av, p->L[4].n, (ntg_av *)p->L[4].av, p->L[5].n, (ntg_av *)p->L[5].av) != 0) return 4;
	printf("SHAPE %d %d %d %d %d\n", n, nc, ldJ0, P, nt);
	for (pt = 0; pt < p->npts; pt++) {
		double *x = p->pts[pt];
		int m, nstate = pt == 0 ? 1 : 0, needc = 0, nn = n, ncc = nc, ldJ = ldJ0;
		printf("POINT %d %d\n", pt, p->full[pt]);
		if (!p->full[pt]) {
			m = 0; F = 0.0; npsolCostFunction(&m, &nn, x, &F, g, &nstate); printf("F0 %.17g\n", F);
			if (nc) { m = 0; npsolConstraintFunction(&m, &ncc, &nn, &ldJ, &needc, x, c, J, &nstate); pvec("C0", c, nc); }
			continue;
		}
		g_rec = rec;
		m = 2; F = 0.0; npsolCostFunction(&m, &nn, x, &F, g, &nstate);
		g_rec = NULL;
		printf("F %.17g\n", F); pvec("G", g, n);
		for (i = 0; i < P && p->nf[4]; i++) { printf("Z %d", i); for (t = 0; t < nt; t++) printf(" %.17g", rec[(size_t)i * nt + t]); printf("\n"); }
		m = 0; F = 0.0; npsolCostFunction(&m, &nn, x, &F, g, &nstate); printf("F0 %.17g\n", F);
		for (i = 0; i < n; i++) g[i] = 0.0;
		m = 1; npsolCostFunction(&m, &nn, x, &F, g, &nstate); pvec("G1", g, n);
		if (nc) {
			for (e = 0; e < (size_t)ldJ0 * n; e++) J[e] = -7.25;
			m = 2; npsolConstraintFunction(&m, &ncc, &nn, &ldJ, &needc, x, c, J, &nstate);
			pvec("C", c, nc); pvec("J", J, (size_t)ldJ0 * n);
		}
		for (o = 0; o < p->nout; o++)
			for (t = 0; t < p->ntimes; t++) {
				SplineInterp(fz, p->times[t], p->knots[o], p->nint[o], x + p->iC[o], p->ncoef[o], p->order[o], p->mult[o], p->md[o]);
				printf("INTERP %d %d", o, t); for (i = 0; i < p->md[o]; i++) printf(" %.17g", fz[i]); printf("\n");
			}
	}
	ntg_close();
	free(g); free(c); free(J); free(rec);
	return 0;
}

static int run_solve(Prob *p)
{
	const int n = p->nC, P = p->nbps, nclin = p->nlin[0] + p->nlin[1] * P + p->nlin[2], nc = p->nf[0] + p->nf[1] * P + p->nf[2], ntot = n + nclin + nc;
	double *coef = calloc(n, sizeof(double)), *clambda = calloc(ntot, sizeof(double)), *R = calloc((size_t)(n + 1) * (n + 1), sizeof(double)), objective = 0.0;
	int *istate = calloc(ntot, sizeof(int)), inform = -1, i;
	G = p;
	memcpy(coef, p->coef, n * sizeof(double));
	ntg(p->nout, p->bps, P, p->nint, p->knots, p->order, p->mult, p->md, coef,
	    p->nlin[0], p->lin[0], p->nlin[1], p->lin[1], p->nlin[2], p->lin[2], p->nf[0], nlicf, p->nf[1], nltcf, p->nf[2], nlfcf,
	    p->L[0].n, p->L[0].av, p->L[1].n, p->L[1].av, p->L[2].n, p->L[2].av, p->lo, p->up,
	    p->nf[3], icf, p->nf[4], ucf, p->nf[5], fcf, p->L[3].n, p->L[3].av, p->L[4].n, p->L[4].av, p->L[5].n, p->L[5].av,
	    istate, clambda, R, &inform, &objective);
	printf("RESULT %d %.17g", inform, objective); for (i = 0; i < n; i++) printf(" %.17g", coef[i]); printf("\n");
	printf("ISTATE"); for (i = 0; i < nclin; i++) printf(" %d", istate[n + i]); printf("\n");
	free(coef); free(clambda); free(R); free(istate);
	return inform;
}

int main(int argc, char **argv)
{
	int i, rc;
	if (argc < 3) die("usage: hostpath_drv eval|solve|sequence FILE [FILE2] [option]...");
	if (!strcmp(argv[1], "eval")) return run_eval(read_problem(argv[2]));
	if (!strcmp(argv[1], "solve")) {
		for (i = 3; i < argc; i++) npsoloption(argv[i]);
		return run_solve(read_problem(argv[2]));
	}
	if (!strcmp(argv[1], "sequence") && argc >= 4) {
		for (i = 4; i < argc; i++) npsoloption(argv[i]);
		rc = run_solve(read_problem(argv[2]));
		rc |= run_solve(read_problem(argv[3]));
		rc |= run_solve(read_problem(argv[2]));
		return rc;
	}
	die("unknown mode");
	return 2;
}
