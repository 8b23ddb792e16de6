/*
 * TEST INFRASTRUCTURE -- CPU oracle for the VFGS firmware layer: what an FGC SEI message or an
 * AFGS1 parameter set programs into the hardware layer, patterns included.  Only tests may load
 * this; the product derives its tables in versatilefilmgrain_amd/csrc/vfgs_fw_host.cpp and makes
 * its patterns on the GPU (vfgs_fw_kernel.hip).
 *
 * This project's own text, in its own structure (as vfgs_oracle.c is for the hardware layer): the
 * *behaviour* of the reference's src/vfgs_fw.c is restated and cited by line number, oddities
 * included (each is marked ODDITY).  Where the reference interleaves list building, pattern making
 * and table filling in one loop over the components, this file builds the two pattern lists
 * first, then emits records bank by bank; where it runs one raster loop per pattern, this file
 * separates the noise term, the filter (a list of non-zero taps) and the crop.  Re-entrant, no
 * globals: the constant tables (Gaussian samples, seeds, 64-point DCT-II basis) are the caller's,
 * the 7168 bytes of versatilefilmgrain_amd/csrc/fw_tables.bin (layout in dump_fw_tables.c).
 *
 * Pinned by tests/test_fw_oracle_c_cpu.py: against the numpy restatement of the two generators
 * (vfgs_fw_oracle.py), against every recorded programming of tests/golden/traces, and -- where the
 * reference is present -- against the real reference firmware over thousands of generated sets.
 *
 * Output of the two init calls: *program records* in the layout of trace_shim.c,
 *   u32 op, i32 a, i32 b, u32 nbytes, payload[nbytes]
 * in the order the reference firmware calls the setters.  A pattern payload is the whole 4096-byte
 * scratch buffer the reference hands over (vfgs_fw.c:519, :666): for a chroma pattern the 32x32
 * pattern in the first 1024 bytes, then the tail of the last luma pattern of the same call.  Where
 * the call made no luma pattern the reference reads an uninitialised stack buffer there; this file
 * writes zeros (the product's choice: fw_commit_chroma, last_luma < 0).
 */
#include <stdint.h>
#include <stdlib.h>
#include <string.h>

#include "../include/vfgs_hip_fw.h"   /* fgs_sei, fgs_afgs1, vfgs_hip_pattern_job: the C layouts only */

enum {
	OP_LUMA_PATTERN = 1, OP_CHROMA_PATTERN = 2, OP_SCALE_LUT = 3, OP_PATTERN_LUT = 4,
	OP_SEED = 5, OP_SCALE_SHIFT = 6, OP_DEPTH = 7, OP_LEGAL_RANGE = 8, OP_CHROMA_SUBSAMPLING = 9
};

#define SLOTS       8      /* pattern slots of a bank, vfgs_hw.h:49 */
#define SCRATCH     4096   /* the 64x64 buffer every pattern is handed over in */
#define TAIL_VALUES (SEI_MAX_MODEL_VALUES - 1)   /* what tells two SEI parameter sets apart: everything but the scale */

typedef struct {
	const int8_t*   gauss;        /* [2048]    vfgs_fw.c:46  */
	const uint32_t* seed;         /* [256]     vfgs_fw.c:177 */
	const int8_t  (*dct)[64];     /* [64][64]  vfgs_fw.c:280 */
} fw_tables;

static fw_tables tables_of(const void* blob)
{
	fw_tables t;
	t.gauss = (const int8_t*)blob;
	t.seed = (const uint32_t*)((const uint8_t*)blob + 2048);
	t.dct = (const int8_t (*)[64])((const uint8_t*)blob + 3072);
	return t;
}

/* ---- record writer ---------------------------------------------------------- */

typedef struct { uint8_t* p; size_t cap, len; int overflow; } recbuf;

static void rec(recbuf* r, uint32_t op, int32_t a, int32_t b, const void* payload, uint32_t n)
{
	if (r->len + 16 + n > r->cap) { r->overflow = 1; r->len += 16 + n; return; }
	memcpy(r->p + r->len, &op, 4);
	memcpy(r->p + r->len + 4, &a, 4);
	memcpy(r->p + r->len + 8, &b, 4);
	memcpy(r->p + r->len + 12, &n, 4);
	if (n) memcpy(r->p + r->len + 16, payload, n);
	r->len += 16 + n;
}

static void rec_scalar(recbuf* r, uint32_t op, int32_t a) { rec(r, op, a, 0, NULL, 0); }
static void rec_table(recbuf* r, uint32_t op, int c, const uint8_t table[256]) { rec(r, op, c, 0, table, 256); }
static void rec_pattern(recbuf* r, int chroma, int slot, const int8_t scratch[SCRATCH])
{
	rec(r, chroma ? OP_CHROMA_PATTERN : OP_LUMA_PATTERN, slot, 0, scratch, SCRATCH);
}

/* ---- small helpers ---------------------------------------------------------- */

static int rshift_round(int v, int s) { return (v + (1 << (s - 1))) >> s; }            /* vfgs_fw.c:43 */
static int clip127(int v) { return v > 127 ? 127 : v < -127 ? -127 : v; }              /* vfgs_fw.c:44 */

/* the firmware's generator is the hardware layer's register (vfgs_fw.c:284-295 = vfgs_hw.c:74-79) */
static uint32_t next_reg(uint32_t reg)
{
	const uint32_t fb = ((reg >> 1) ^ (reg >> 29)) & 1u;
	return (reg >> 1) | (fb << 31);
}

/* ---- frequency-filtered pattern: vfgs_fw.c:362-408 (fill) + :297-360 (two basis passes) ---- */

/* One basis pass over an n x n block: out[r][c] = (round + sum_k left(r,k) * right(k,c)) >> shift, where one side is the block and the
 * other the (n-point) basis; the 32-point basis is every other row of the 64-point one (vfgs_fw.c:343, :354). */
static void ff_pattern(const fw_tables* t, int n, int cut_h, int cut_v, uint32_t reg, int8_t* out)
{
	const int per_step = n / 16;                  /* samples drawn per generator step: 4 (luma) or 2 (chroma) */
	const int basis_step = 64 / n;
	const int cols = per_step * (cut_h + 1), rows = per_step * (cut_v + 1);   /* the low-frequency corner that holds noise */
	int8_t coef[64][64];
	int16_t mid[64][64];
	int g, s, r, c, k;

	/* the generator steps once per group of per_step samples, inside the corner or not; 16 groups per row */
	memset(coef, 0, sizeof coef);
	for (g = 0; g < 16 * n; g++, reg = next_reg(reg))
	{
		const int row = g / 16, col = (g % 16) * per_step;
		if (row >= rows || col >= cols)
			continue;
		for (s = 0; s < per_step; s++)
			coef[row][col + s] = t->gauss[(reg + (uint32_t)s) & 2047];
	}
	coef[0][0] = 0;                               /* no DC */

	/* columns first (the basis transposed), 9 bits of headroom dropped at 64 points and 8 at 32 ... */
	for (r = 0; r < n; r++)
		for (c = 0; c < n; c++)
		{
			int32_t sum = 0;
			for (k = 0; k < n; k++)
				sum += (int32_t)t->dct[k * basis_step][r] * coef[k][c];
			mid[r][c] = (int16_t)(n == 64 ? (sum + 256) >> 9 : (sum + 128) >> 8);
		}
	/* ... then rows, always 9 bits, clipped to +-127 */
	for (r = 0; r < n; r++)
		for (c = 0; c < n; c++)
		{
			int32_t sum = 0;
			for (k = 0; k < n; k++)
				sum += (int32_t)mid[r][k] * t->dct[k * basis_step][c];
			out[r * n + c] = (int8_t)clip127((sum + 256) >> 9);
		}
}

/* ---- auto-regressive pattern: vfgs_fw.c:464-501 on a 4x7 tap matrix laid out as :412 ---- */

typedef struct { int offset; int weight; } ar_tap;   /* offset into the working buffer relative to the sample */

/* The taps that can matter: the causal half of the matrix (rows above, and the sample's own row left of it), zeros dropped.
 * Row 3 of the matrix is the sample's row, column 3 the sample's column. */
static int causal_taps(const int16_t matrix[28], int width, ar_tap taps[24])
{
	int n = 0, cell;
	for (cell = 0; cell < 3 * 7 + 3; cell++)
		if (matrix[cell])
		{
			taps[n].offset = (cell / 7 - 3) * width + (cell % 7 - 3);
			taps[n].weight = matrix[cell];
			n++;
		}
	return n;
}

static void ar_pattern(const fw_tables* t, int size, const int16_t matrix[28], int noise_shift, int sum_shift, uint32_t reg, int8_t* out)
{
	const int chroma = size == 32;
	const int width = chroma ? 44 : 82, height = chroma ? 38 : 73;   /* the working buffer, vfgs_fw.c:422-423 */
	const int margin = 3;                                              /* the filter's reach: no filtering closer to the border */
	const int origin = margin + (chroma ? 3 : 6);                      /* where the kept window begins, vfgs_fw.c:498-501 */
	int8_t work[73 * 82];
	ar_tap taps[24];
	const int ntaps = causal_taps(matrix, width, taps);
	int pos, k, row;

	/* the noise term of every sample: one generator step per sample in raster order, vfgs_fw.c:491-492 */
	for (pos = 0; pos < width * height; pos++, reg = next_reg(reg))
		work[pos] = (int8_t)rshift_round(t->gauss[reg & 2047], noise_shift);
	/* the recursion in raster order; each sample replaces its own noise term */
	for (pos = 0; pos < width * height; pos++)
	{
		const int y = pos / width, x = pos % width;
		int v = work[pos];
		if (y >= margin && x >= margin && x < width - margin)
		{
			int sum = 0;
			for (k = 0; k < ntaps; k++)
				sum += taps[k].weight * work[pos + taps[k].offset];
			v += rshift_round(sum, sum_shift);
		}
		work[pos] = (int8_t)clip127(v);
	}
	for (row = 0; row < size; row++)
		memcpy(out + row * size, work + (origin + row) * width + origin, (size_t)size);
}

/* SEI auto-regressive model values -> taps (vfgs_fw.c:427-436): first- and second-order correlation to the left, the same upwards scaled
 * by the aspect value v[4], the diagonals from v[3].  ODDITY: the taps are stored as int16, products included. */
static void sei_ar_taps(const int16_t* v, int scale, int16_t matrix[28])
{
	enum { UP2 = 1 * 7 + 3, UP_LEFT = 2 * 7 + 2, UP = 2 * 7 + 3, UP_RIGHT = 2 * 7 + 4, LEFT2 = 3 * 7 + 1, LEFT = 3 * 7 + 2 };
	const int32_t horizontal = v[1], diagonal = v[3], aspect = v[4], second = v[5];
	const int16_t diag = (int16_t)((diagonal * aspect) >> scale);
	memset(matrix, 0, 28 * sizeof(int16_t));
	matrix[LEFT] = (int16_t)horizontal;
	matrix[LEFT2] = (int16_t)second;
	matrix[UP] = (int16_t)((horizontal * aspect) >> scale);
	matrix[UP_LEFT] = matrix[UP_RIGHT] = diag;
	matrix[UP2] = (int16_t)((int32_t)((uint32_t)second * (uint32_t)aspect * (uint32_t)aspect) >> (2 * scale));
}

/* AV1 coefficient order -> taps (vfgs_fw.c:459-462): the causal neighbourhood of reach `lag` in raster order, lag full rows of
 * 2 lag + 1 and then the lag samples to the left */
static void afgs1_taps(const int16_t* ar, int lag, int16_t matrix[28])
{
	const int span = 2 * lag + 1, count = 2 * lag * (lag + 1);
	int pos;
	memset(matrix, 0, 28 * sizeof(int16_t));
	for (pos = 0; pos < count; pos++)
		matrix[(3 - lag + pos / span) * 7 + (3 - lag + pos % span)] = ar[pos];
}

/* One pattern from a job with the fields of vfgs_hip_pattern_job: n*n bytes (n = 64 luma, 32 chroma) into out.
 * Returns n*n, or -1 for a job outside what the generators define. */
int vfgs_fw_oracle_pattern(const void* blob, const vfgs_hip_pattern_job* job, signed char* out)
{
	const fw_tables t = tables_of(blob);
	const int n = job->chroma ? 32 : 64;
	if (job->seed_index < 0 || job->seed_index > 255) return -1;
	if (job->kind == 0)
		ff_pattern(&t, n, job->fh, job->fv, t.seed[job->seed_index], (int8_t*)out);
	else if (job->kind == 1)
	{
		if (job->scale < 1 || job->scale > 30 || job->shift < 1 || job->shift > 30) return -1;
		ar_pattern(&t, n, job->coef, job->shift, job->scale, t.seed[job->seed_index], (int8_t*)out);
	}
	else
		return -1;
	return n * n;
}

/* ---- vfgs_init_sei: vfgs_fw.c:517-644 ---------------------------------------- */

/* The distinct parameter sets of one bank, in slot order.  An entry names an interval (component, index); slots at and beyond `used`
 * are empty. */
typedef struct {
	int used;
	struct { uint8_t lower; uint8_t comp; uint16_t interval; } slot[SLOTS];
} sei_list;

static const int16_t* sei_values(const fgs_sei* cfg, int comp, int interval) { return cfg->comp_model_value[comp][interval]; }

/* What the reference's search compares an interval against at slot i (vfgs_fw.c:504-514, :537).  ODDITY: an empty slot is not skipped: it
 * compares as the FIRST five numbers of luma's first interval, scale included. */
static const int16_t* slot_tail(const fgs_sei* cfg, const sei_list* list, int i)
{
	if (i < list->used)
		return sei_values(cfg, list->slot[i].comp, list->slot[i].interval) + 1;
	return sei_values(cfg, 0, 0);
}

/* the first slot whose tail equals the interval's, SLOTS if none */
static int slot_of(const fgs_sei* cfg, const sei_list* list, int comp, int interval)
{
	const int16_t* tail = sei_values(cfg, comp, interval) + 1;
	int i = 0;
	while (i < SLOTS && memcmp(slot_tail(cfg, list, i), tail, TAIL_VALUES * sizeof(int16_t)))
		i++;
	return i;
}

/* vfgs_fw.c:540-570: an interval whose tail no slot matches joins the list behind the entries whose lower bound is not above its own.
 * ODDITY: a full list takes no more; such an interval ends up without a slot. */
static void sei_collect(const fgs_sei* cfg, sei_list* list, int comp)
{
	int interval, at;
	if (!cfg->comp_model_present_flag[comp])
		return;
	for (interval = 0; interval < cfg->num_intensity_intervals[comp]; interval++)
	{
		const uint8_t lower = cfg->intensity_interval_lower_bound[comp][interval];
		if (list->used == SLOTS || slot_of(cfg, list, comp, interval) != SLOTS)
			continue;
		at = list->used++;
		while (at > 0 && list->slot[at - 1].lower > lower)
		{
			list->slot[at] = list->slot[at - 1];
			at--;
		}
		list->slot[at].lower = lower;
		list->slot[at].comp = (uint8_t)comp;
		list->slot[at].interval = (uint16_t)interval;
	}
}

/* vfgs_fw.c:600-635: the two tables of a component.  `scale` is written only inside the component's intervals (what it held shows through
 * the gaps); `select` is written whole: the slot in bits 7:4 inside the intervals that have one, and every other intensity repeats the
 * entry below it (ODDITY: no interpolation; 0 below the first). */
static void sei_tables(const fgs_sei* cfg, const sei_list* list, int comp, uint8_t scale[256], uint8_t select[256])
{
	uint8_t known[256];
	int interval, v;
	memset(select, 0, 256);
	if (!cfg->comp_model_present_flag[comp])
		return;
	memset(known, 0, sizeof known);
	for (interval = 0; interval < cfg->num_intensity_intervals[comp]; interval++)
	{
		const int first = cfg->intensity_interval_lower_bound[comp][interval];
		const int last = cfg->intensity_interval_upper_bound[comp][interval];       /* below `first`: an empty interval */
		const int slot = slot_of(cfg, list, comp, interval);
		for (v = first; v <= last; v++)
		{
			scale[v] = (uint8_t)sei_values(cfg, comp, interval)[0];
			if (slot < SLOTS)
			{
				select[v] = (uint8_t)(slot << 4);
				known[v] = 1;
			}
		}
	}
	for (v = 1; v < 256; v++)
		if (!known[v])
			select[v] = select[v - 1];
}

/* the patterns of a list into records, slot by slot; the scratch buffer is shared by the whole call */
static void sei_patterns(const fw_tables* t, const fgs_sei* cfg, const sei_list* list, int chroma, int8_t scratch[SCRATCH], recbuf* r)
{
	const int size = chroma ? 32 : 64;
	const uint32_t start = t->seed[chroma];       /* vfgs_fw.c:369, :394, :581, :590 */
	int16_t matrix[28];
	int i;
	for (i = 0; i < list->used; i++)
	{
		const int16_t* v = sei_values(cfg, list->slot[i].comp, list->slot[i].interval);
		if (cfg->model_id)
		{
			sei_ar_taps(v, cfg->log2_scale_factor, matrix);
			ar_pattern(t, size, matrix, 1, cfg->log2_scale_factor, start, scratch);
		}
		else
			ff_pattern(t, size, v[1], v[2], start, scratch);
		rec_pattern(r, chroma, i, scratch);       /* (a chroma pattern fills 1024 bytes: what a luma pattern left behind them stays) */
	}
}

long vfgs_fw_oracle_init_sei(const void* blob, const fgs_sei* cfg, void* out, size_t cap)
{
	const fw_tables t = tables_of(blob);
	recbuf r = { (uint8_t*)out, cap, 0, 0 };
	int8_t scratch[SCRATCH];
	uint8_t scale[256], select[256];
	sei_list luma, chroma;
	int comp;

	if (cfg->model_id && (cfg->log2_scale_factor < 1 || cfg->log2_scale_factor > 15)) return -1;   /* a shift by 0 bits - 1: undefined in the reference */
	for (comp = 0; comp < 3; comp++)
		if (cfg->comp_model_present_flag[comp] && cfg->num_intensity_intervals[comp] > 256) return -1;   /* the arrays hold 256 */

	memset(&luma, 0, sizeof luma);
	memset(&chroma, 0, sizeof chroma);
	sei_collect(cfg, &luma, 0);
	sei_collect(cfg, &chroma, 1);                 /* Cb and Cr share one bank and one list, vfgs_fw.c:533-538 */
	sei_collect(cfg, &chroma, 2);

	memset(scratch, 0, sizeof scratch);           /* uninitialised in the reference; zeros are this project's documented choice */
	sei_patterns(&t, cfg, &luma, 0, scratch, &r);
	memset(scale, 0, sizeof scale);
	sei_tables(cfg, &luma, 0, scale, select);
	rec_table(&r, OP_SCALE_LUT, 0, scale);
	rec_table(&r, OP_PATTERN_LUT, 0, select);

	sei_patterns(&t, cfg, &chroma, 1, scratch, &r);
	memset(scale, 0, sizeof scale);               /* ODDITY: cleared in front of Cb only: Cr shows Cb's scales through its gaps (vfgs_fw.c:532, :598) */
	for (comp = 1; comp < 3; comp++)
	{
		sei_tables(cfg, &chroma, comp, scale, select);
		rec_table(&r, OP_SCALE_LUT, comp, scale);
		rec_table(&r, OP_PATTERN_LUT, comp, select);
	}
	rec_scalar(&r, OP_SCALE_SHIFT, cfg->log2_scale_factor - (cfg->model_id ? 1 : 0));   /* the auto-regressive noise is drawn at shift 1 */
	return r.overflow ? -2 : (long)r.len;
}

/* ---- vfgs_init_afgs1: vfgs_fw.c:649-708 -------------------------------------- */

/* the scaling function of vfgs_fw.c:649-660: zero outside the points, every segment written end points included (so a later segment
 * rewrites the shared point with its own start value), C's truncating division also on falling segments.  -1: points not increasing */
static int scaling_function(uint8_t table[256], const uint8_t* x, const uint8_t* y, int npoints)
{
	int seg, t;
	memset(table, 0, 256);
	for (seg = 0; seg + 1 < npoints; seg++)
	{
		const int x0 = x[seg], x1 = x[seg + 1], y0 = y[seg], rise = (int)y[seg + 1] - y0, span = x1 - x0;
		if (span <= 0) return -1;                 /* the reference asserts */
		for (t = x0; t <= x1; t++)
			table[t] = (uint8_t)(y0 + (rise * (t - x0) + span / 2) / span);
	}
	return 0;
}

long vfgs_fw_oracle_init_afgs1(const void* blob, const fgs_afgs1* cfg, void* out, size_t cap)
{
	const fw_tables t = tables_of(blob);
	recbuf r = { (uint8_t*)out, cap, 0, 0 };
	const struct { const int16_t* ar; const uint8_t* x; const uint8_t* y; int npoints; int slot; int select; } comp[3] = {
		{ cfg->ar_coeffs_y,  cfg->point_y_values,  cfg->point_y_scaling,  cfg->num_y_points,  0, 0 },
		{ cfg->ar_coeffs_cb, cfg->point_cb_values, cfg->point_cb_scaling, cfg->num_cb_points, 0, 0 },
		/* ODDITY: Cr's pattern goes to chroma slot 1 and its pattern LUT is filled with 1 -- slot 0 (the slot is bits 7:4) */
		{ cfg->ar_coeffs_cr, cfg->point_cr_values, cfg->point_cr_scaling, cfg->num_cr_points, 1, 1 },
	};
	const int lag = cfg->ar_coeff_lag;
	uint8_t table[256];
	int8_t scratch[SCRATCH];
	int16_t matrix[28];
	int c;

	if (lag < 1 || lag > 3) return -1;            /* the reference asserts on any other tap count, vfgs_fw.c:457 */
	if (cfg->num_y_points > 14 || cfg->num_cb_points > 10 || cfg->num_cr_points > 10) return -1;
	if (cfg->ar_coeff_shift < 1 || cfg->ar_coeff_shift > 15) return -1;

	rec_scalar(&r, OP_SEED, (int32_t)(cfg->grain_seed * 0x10001u));   /* the 16-bit seed in both halves, vfgs_fw.c:672 */
	for (c = 0; c < 3; c++)
	{
		/* with chroma_scaling_from_luma Cb and Cr take luma's table as it stands (vfgs_fw.c:677-682) */
		if ((c == 0 || !cfg->chroma_scaling_from_luma) && scaling_function(table, comp[c].x, comp[c].y, comp[c].npoints))
			return -1;
		rec_table(&r, OP_SCALE_LUT, c, table);
	}
	for (c = 0; c < 3; c++)
	{
		/* ODDITY: all three filters read 2 lag (lag + 1) values (vfgs_fw.c:688); the chroma filters' extra value, luma's weight, is never used */
		afgs1_taps(comp[c].ar, lag, matrix);
		ar_pattern(&t, c ? 32 : 64, matrix, cfg->grain_scale_shift + 1, cfg->ar_coeff_shift, t.seed[c], scratch);   /* chroma: the luma pattern's tail stays */
		rec_pattern(&r, c > 0, comp[c].slot, scratch);
		memset(table, comp[c].select, sizeof table);
		rec_table(&r, OP_PATTERN_LUT, c, table);
	}
	rec_scalar(&r, OP_SCALE_SHIFT, cfg->grain_scaling - 6);
	rec_scalar(&r, OP_LEGAL_RANGE, cfg->clip_to_restricted_range);
	return r.overflow ? -2 : (long)r.len;
}
