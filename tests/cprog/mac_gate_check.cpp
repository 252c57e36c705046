// tests/cprog/mac_gate_check.cpp -- pirip_amd/csrc/mac_device.hpp on the host, against the table tests/macref.py writes (argv[1]):
//   R <slot_calls> <cw> <key>                                  the rules of the G lines that follow
//   D <key> <t> <a> <cw> <draw>
//   G <ifs_calls> <txop_bursts> <phase> <counter> <run> <due> <queued> <idle> | <phase> <counter> <run> <accesses> <won> <backoff>
//     <deferred> <limit>                                        channel 5 at access 7
// Prints the lines checked; exit status 1 and the first line that differs otherwise. tests/test_mac_cpu.py also builds this file with
// -fsanitize=address,undefined.
#include <cstdio>
#include <cstdlib>
#include <cstring>

#include "mac_device.hpp"

int main(int argc, char **argv)
{
    if (argc != 2) return 2;
    FILE *f = fopen(argv[1], "r");
    if (!f) return 2;
    char *line = (char *)malloc(256);
    if (!line) return 2;
    pirip::MacRules r{1, 1, 0, 1, 0u};
    long draws = 0, gates = 0;
    int rc = 0;
    while (!rc && fgets(line, 256, f)) {
        if (line[0] == 'R') {
            unsigned key = 0;
            if (sscanf(line, "R %d %d %u", &r.slot_calls, &r.cw, &key) != 3) rc = 2;
            r.key = key;
        } else if (line[0] == 'D') {
            unsigned key = 0, t = 0, a = 0, cw = 0;
            int want = -1;
            if (sscanf(line, "D %u %u %u %u %d", &key, &t, &a, &cw, &want) != 5) rc = 2;
            else if (pirip::mac_draw(key, t, a, cw) != want) rc = 1;
            draws++;
        } else if (line[0] == 'G') {
            int in[8], out[8];
            if (sscanf(line, "G %d %d %d %d %d %d %d %d | %d %d %d %d %d %d %d %d", &in[0], &in[1], &in[2], &in[3], &in[4], &in[5], &in[6], &in[7], &out[0],
                       &out[1], &out[2], &out[3], &out[4], &out[5], &out[6], &out[7]) != 16) {
                rc = 2;
                break;
            }
            r.ifs_calls = in[0]; r.txop_bursts = in[1];
            pirip::MacGate g{in[2], in[3], in[4], 7, 0, 0, 0};
            const int limit = pirip::mac_gate_step(g, r, 5, in[5] != 0, in[6] != 0, in[7]);
            const long long got[8] = {g.phase, g.counter, g.run, g.accesses, g.won, g.backoff, g.deferred, limit};
            for (int i = 0; i < 8; i++)
                if (got[i] != out[i]) rc = 1;
            gates++;
        } else if (line[0] != '\n') {
            rc = 2;
        }
        if (rc) fprintf(stderr, "differs (%d): %s", rc, line);
    }
    // the runs stop counting where the header says
    if (pirip::mac_run_next(pirip::kMacRunMax, false) != pirip::kMacRunMax || pirip::mac_run_next(pirip::kMacRunMax - 1, false) != pirip::kMacRunMax ||
        pirip::mac_run_next(5, true) != 0 || pirip::mac_run_next(0, false) != 1)
        rc = 1;
    free(line);
    fclose(f);
    printf("draws %ld gates %ld\n", draws, gates);
    return rc;
}
