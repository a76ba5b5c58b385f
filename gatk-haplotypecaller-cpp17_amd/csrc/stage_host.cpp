// The registry of the stage engines' Stages (stage_host.hpp) and their release.
#include "stage_host.hpp"

namespace stage_host {

std::vector<Stage*>& stages()
{
    static std::vector<Stage*> v;
    return v;
}

// The order needs no encoding: every stage call drains its stream before it
// returns, each release takes its stage's lock, and a stage that works on
// another's stream (the contig caller on the parser's) holds that stage's lock
// while it does.
void release_all()
{
    for (Stage* s : stages()) s->release();
}

}  // namespace stage_host
